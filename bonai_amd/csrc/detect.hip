// detect.hip -- the RoI head's detection selection (mmdet/core/post_processing/bbox_nms.py:5-69, multiclass_nms) for the B images of a
// batch at once, with no decision taken on the host between its steps.
//
// The per-image path (LoftRoIHead.multiclass_nms) indexes with a boolean mask, asks whether anything is left, reads a maximum and
// uploads a segment table: each of those stops the queue.  Here the same selection is four small launches around the existing sort,
// NMS and top-k kernels of nms.hip, all sized from what the host knows beforehand (rows R, classes C, rows of the largest image):
//
//   loft_det_candidates    scores > score_thr, compacted IN ORDER into one segment per (image, class), image-major, ascending flat
//                          index row * C + class inside a segment; segment offsets, each image's coordinate maximum (batched_nms's
//                          `boxes.max()`), a flag per flat index, and the class scores as a dense [R * C] array
//   (loft_segmented_sort_desc over the segments, values = flat indices)
//   loft_det_gather_boxes  the sorted candidates' boxes, for loft_nms_segmented_levels (classes are its "levels")
//   loft_det_scatter_keep  the keep flags back to flat-index positions
//   (loft_segmented_topk_desc per image over the dense scores with those flags as key mask: score descending ACROSS classes, ties by
//    ascending flat index -- the order `dets[:max_num]` of the per-image path cuts)
//   loft_det_finalize      dets / labels / counts per image and the detections' RoIs, compact and image-major
//
// Order never depends on arrival: positions come from wave64 ballots and prefix counts, sums over earlier segments are recomputed by
// every workgroup from a count table written by the launch before.  No atomics.  Values are copied, never recomputed: a detection
// carries the bits of its box and score.
#include "loft_common.h"
#include "../../include/loft_hip.h"

#define DET_THREADS 256
#define DET_WAVES (DET_THREADS / 64)

namespace {

// torch's max propagates NaN: so does this
__device__ __forceinline__ float det_nanmax(float a, float b) { return a != a ? a : (b != b ? b : fmaxf(a, b)); }

__device__ __forceinline__ int det_block_sum(int v, int* ws) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();                                   // ws may still be read from the previous call
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < DET_WAVES; ++w) s += ws[w];
    return s;
}

__device__ __forceinline__ float det_block_nanmax(float v, float* ws) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = det_nanmax(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = ws[0];
#pragma unroll
    for (int w = 1; w < DET_WAVES; ++w) s = det_nanmax(s, ws[w]);
    return s;
}

__device__ __forceinline__ float4 det_box(const float* __restrict__ bboxes, int box_cols, long row, int c) {
    return *reinterpret_cast<const float4*>(bboxes + row * box_cols + (box_cols == 4 ? 0 : 4 * c));
}

}  // namespace

// grid: one workgroup per (image, class) segment.  -> seg_count[seg], seg_max[seg] (the maximum over its candidates' coordinates)
__global__ __launch_bounds__(DET_THREADS) void det_count_kernel(const float* __restrict__ scores, const float* __restrict__ bboxes,
                                                              const int64_t* __restrict__ roi_off, int C, int box_cols, float thr,
                                                              int* __restrict__ seg_count, float* __restrict__ seg_max) {
    __shared__ int wsi[DET_WAVES];
    __shared__ float wsf[DET_WAVES];
    const int seg = blockIdx.x, b = seg / C, c = seg % C;
    const long r0 = roi_off[b], r1 = roi_off[b + 1];
    int n = 0;
    float m = -INFINITY;
    for (long r = r0 + threadIdx.x; r < r1; r += DET_THREADS) {
        if (scores[r * (C + 1) + c] > thr) {
            ++n;
            const float4 q = det_box(bboxes, box_cols, r, c);
            m = det_nanmax(det_nanmax(det_nanmax(m, q.x), det_nanmax(q.y, q.z)), q.w);
        }
    }
    n = det_block_sum(n, wsi);
    m = det_block_nanmax(m, wsf);
    if (threadIdx.x == 0) { seg_count[seg] = n; seg_max[seg] = m; }
}

// grid: one workgroup per segment.  Its first candidate lands at the sum of the counts of the segments before it; inside the segment
// candidates keep row order: per 256 rows, a ballot per wave, the lanes below in the ballot, the waves below in the workgroup.
__global__ __launch_bounds__(DET_THREADS) void det_compact_kernel(const float* __restrict__ scores, const int64_t* __restrict__ roi_off,
                                                                int B, int C, float thr, int64_t cap,
                                                                const int* __restrict__ seg_count, const float* __restrict__ seg_max,
                                                                int64_t* __restrict__ seg_off, float* __restrict__ img_max,
                                                                uint8_t* __restrict__ flag, float* __restrict__ score_flat,
                                                                float* __restrict__ cand_score, int32_t* __restrict__ cand_flat) {
    __shared__ int wsi[DET_WAVES];
    __shared__ int wcnt[DET_WAVES];
    const int S = B * C, seg = blockIdx.x, b = seg / C, c = seg % C;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int before = 0, all = 0;
    for (int s = tid; s < S; s += DET_THREADS) {
        const int v = seg_count[s];
        all += v;
        before += s < seg ? v : 0;
    }
    before = det_block_sum(before, wsi);
    all = det_block_sum(all, wsi);
    if (tid == 0) {
        seg_off[seg] = before;
        if (seg == S - 1) { seg_off[S] = all; seg_off[S + 1] = cap; }     // the rest of the arrays: a segment the sort may order, nothing reads
        if (c == 0) {                                                     // batched_nms's boxes.max() of image b
            float m = -INFINITY;
            for (int q = 0; q < C; ++q)
                if (seg_count[b * C + q] > 0) m = det_nanmax(m, seg_max[b * C + q]);
            img_max[b] = m == -INFINITY ? 0.f : m;                        // no candidate: nothing reads it
        }
    }
    for (long i = (long)all + (long)seg * DET_THREADS + tid; i < cap; i += (long)S * DET_THREADS) {
        cand_score[i] = -1.f;
        cand_flat[i] = 0;
    }
    const long r0 = roi_off[b], r1 = roi_off[b + 1];
    long pos = before;
    for (long rb = r0; rb < r1; rb += DET_THREADS) {                      // wave-uniform trip count
        const long r = rb + tid;
        const float sc = r < r1 ? scores[r * (C + 1) + c] : 0.f;
        const bool is = r < r1 && sc > thr;
        const unsigned long long bal = __ballot(is);
        if (lane == 0) wcnt[wave] = __popcll(bal);
        __syncthreads();
        int below = 0, chunk = 0;
#pragma unroll
        for (int w = 0; w < DET_WAVES; ++w) { below += w < wave ? wcnt[w] : 0; chunk += wcnt[w]; }
        if (r < r1) {
            const long f = r * C + c;
            flag[f] = is ? 1 : 0;
            score_flat[f] = sc;
            if (is) {
                const long p = pos + below + __popcll(bal & ((1ull << lane) - 1ull));
                cand_score[p] = sc;
                cand_flat[p] = (int32_t)f;
            }
        }
        pos += chunk;
        __syncthreads();
    }
}

LOFT_EXPORT int loft_det_candidates(const float* scores, const float* bboxes, int box_cols, const int64_t* roi_off_dev, int B, int C,
                                    int64_t R, float score_thr, int32_t* work, int64_t* seg_off, float* img_max, uint8_t* flag,
                                    float* score_flat, float* cand_score, int32_t* cand_flat, void* stream) {
    if (B < 1 || C < 1 || R < 0 || (box_cols != 4 && box_cols != 4 * C) || R * C > 0x7fffffffL) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const int S = B * C;
    int* seg_count = work;
    float* seg_max = reinterpret_cast<float*>(work + S);
    hipLaunchKernelGGL(det_count_kernel, dim3(S), dim3(DET_THREADS), 0, s, scores, bboxes, roi_off_dev, C, box_cols, score_thr,
                       seg_count, seg_max);
    LOFT_LAUNCH_CHECK();
    hipLaunchKernelGGL(det_compact_kernel, dim3(S), dim3(DET_THREADS), 0, s, scores, roi_off_dev, B, C, score_thr, R * C, seg_count,
                       seg_max, seg_off, img_max, flag, score_flat, cand_score, cand_flat);
    LOFT_LAUNCH_CHECK();
    return 0;
}

// sorted position i < total (= seg_off[S], read on the device) -> the box of flat index sorted_flat[i]; zeros past the candidates
__global__ __launch_bounds__(DET_THREADS) void det_gather_kernel(const float* __restrict__ bboxes, int box_cols, int C,
                                                               const int32_t* __restrict__ sorted_flat,
                                                               const int64_t* __restrict__ total_p, int64_t cap,
                                                               float* __restrict__ out) {
    const long i = (long)blockIdx.x * DET_THREADS + threadIdx.x;
    if (i >= cap) return;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < *total_p) {
        const int f = sorted_flat[i];
        q = det_box(bboxes, box_cols, f / C, f % C);
    }
    reinterpret_cast<float4*>(out)[i] = q;
}

LOFT_EXPORT int loft_det_gather_boxes(const float* bboxes, int box_cols, int C, const int32_t* sorted_flat, const int64_t* seg_off,
                                      int num_segments, int64_t cap, float* boxes_sorted, void* stream) {
    if (C < 1 || (box_cols != 4 && box_cols != 4 * C) || num_segments < 1) return (int)hipErrorInvalidValue;
    if (cap <= 0) return 0;
    hipLaunchKernelGGL(det_gather_kernel, dim3(loft_cdiv(cap, DET_THREADS)), dim3(DET_THREADS), 0, (hipStream_t)stream, bboxes,
                       box_cols, C, sorted_flat, seg_off + num_segments, cap, boxes_sorted);
    LOFT_LAUNCH_CHECK();
    return 0;
}

__global__ __launch_bounds__(DET_THREADS) void det_scatter_kernel(const uint8_t* __restrict__ keep, const int32_t* __restrict__ sorted_flat,
                                                                const int64_t* __restrict__ total_p, uint8_t* __restrict__ flag) {
    const long i = (long)blockIdx.x * DET_THREADS + threadIdx.x;
    if (i < *total_p) flag[sorted_flat[i]] = keep[i];
}

LOFT_EXPORT int loft_det_scatter_keep(const uint8_t* keep_sorted, const int32_t* sorted_flat, const int64_t* seg_off, int num_segments,
                                      int64_t cap, uint8_t* flag, void* stream) {
    if (num_segments < 1) return (int)hipErrorInvalidValue;
    if (cap <= 0) return 0;
    hipLaunchKernelGGL(det_scatter_kernel, dim3(loft_cdiv(cap, DET_THREADS)), dim3(DET_THREADS), 0, (hipStream_t)stream, keep_sorted,
                       sorted_flat, seg_off + num_segments, flag);
    LOFT_LAUNCH_CHECK();
    return 0;
}

// grid: one workgroup per image.  top_keys / top_vals: loft_segmented_topk_desc's layout over the dense scores, segment b at
// roi_off[b] * C; the survivors lead it (a masked key counts as -1, a candidate's score is above it), so image b's detections are its
// first count_b entries, count_b = those of the first min(k, rows_b * C) whose flag is set.
__global__ __launch_bounds__(DET_THREADS) void det_finalize_kernel(const float* __restrict__ top_keys, const int32_t* __restrict__ top_vals,
                                                                 const uint8_t* __restrict__ flag, const float* __restrict__ bboxes,
                                                                 int box_cols, const int64_t* __restrict__ roi_off, int B, int C, int k,
                                                                 float* __restrict__ dets, int64_t* __restrict__ labels,
                                                                 int64_t* __restrict__ counts, float* __restrict__ rois) {
    __shared__ int wsi[DET_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    int mine = 0, before = 0, all = 0;
    for (int q = 0; q < B; ++q) {                                        // every workgroup counts every image: B * k flag reads
        const long base = roi_off[q] * C;
        const long nq = (roi_off[q + 1] - roi_off[q]) * C;
        const int kk = (int)(nq < k ? nq : k);
        int n = 0;
        for (int r = tid; r < kk; r += DET_THREADS) n += flag[top_vals[base + r]] ? 1 : 0;
        n = det_block_sum(n, wsi);
        all += n;
        before += q < b ? n : 0;
        mine = q == b ? n : mine;
    }
    if (tid == 0) counts[b] = mine;
    const long base = roi_off[b] * C;
    for (int r = tid; r < k; r += DET_THREADS) {
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        float sc = 0.f;
        int c = 0;
        if (r < mine) {
            const int f = top_vals[base + r];
            c = f % C;
            q = det_box(bboxes, box_cols, f / C, c);
            sc = top_keys[base + r];
            float* ro = rois + (long)(before + r) * 5;
            ro[0] = (float)b; ro[1] = q.x; ro[2] = q.y; ro[3] = q.z; ro[4] = q.w;
        }
        float* d = dets + ((long)b * k + r) * 5;
        d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w; d[4] = sc;
        labels[(long)b * k + r] = c;
    }
    for (long i = (long)all * 5 + (long)b * DET_THREADS + tid; i < (long)B * k * 5; i += (long)B * DET_THREADS) rois[i] = 0.f;
}

LOFT_EXPORT int loft_det_finalize(const float* top_keys, const int32_t* top_vals, const uint8_t* keep_flat, const float* bboxes,
                                  int box_cols, const int64_t* roi_off_dev, int B, int C, int max_per_img, float* dets,
                                  int64_t* labels, int64_t* counts, float* rois, void* stream) {
    if (B < 1 || C < 1 || max_per_img < 1 || (box_cols != 4 && box_cols != 4 * C)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(det_finalize_kernel, dim3(B), dim3(DET_THREADS), 0, (hipStream_t)stream, top_keys, top_vals, keep_flat, bboxes,
                       box_cols, roi_off_dev, B, C, max_per_img, dets, labels, counts, rois);
    LOFT_LAUNCH_CHECK();
    return 0;
}
