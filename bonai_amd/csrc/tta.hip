// tta.hip -- test-time augmentation over the symmetries of the square: the merges of mmdet/core/post_processing/merge_augs.py and
// of the RoI head's aug_test_* mixins (mmdet/models/roi_heads/test_mixins.py:74-107,179-208, dense_heads/rpn_test_mixin.py:40-60) as
// five launches for all views, nothing leaving the device.
//
// A view is one element of the square's symmetry group in the encoding of loft_image_prep_d4 (include/loft_hip.h LOFT_D4_*): an
// optional transpose, then an optional x-mirror, then an optional y-mirror.  Every kernel reads the elements of the V views from a
// small DEVICE table (int32 [V]).  img_h x img_w is the ORIGINAL tile; a transposing view's image is img_w x img_h.
//   box into a view:   transpose swaps (x, y); x-mirror: x1' = Wv - x2, x2' = Wv - x1; y-mirror alike with Hv -- the reference's
//                      bbox_flip (mmdet/core/bbox/transforms.py:5-27) in fp32, in that order; scale factor 1 (fixed-size tiles)
//   box back:          the same steps undone in reverse order (y-mirror, x-mirror, transpose); every step is its own inverse
//   offset vector back: y-mirror negates y, x-mirror negates x, transpose swaps the components
//   S x S mask grid back: original tap (r, c) is the view's tap (y, x), (y', x') = T ? (c, r) : (r, c), x = MX ? S-1-x' : x', y alike
// A mean over views is a sequential fp32 sum in view order divided by V (what torch.stack(...).mean(0) and np.mean(axis=0) compute
// on the host for V <= 8).  Wave64 kernels, no atomics, plain C++ stores; built with -ffp-contract=off like boxes.hip.
#include "loft_common.h"
#include "box_codec.h"
#include "../../include/loft_hip.h"

#define TTA_MAX_VIEWS 8

struct ViewDims { float wv, hv; };
__device__ __forceinline__ ViewDims view_dims(int e, int img_h, int img_w) {
    ViewDims d;
    d.wv = (float)((e & LOFT_D4_TRANSPOSE) ? img_h : img_w);
    d.hv = (float)((e & LOFT_D4_TRANSPOSE) ? img_w : img_h);
    return d;
}
__device__ __forceinline__ float4 box_to_view(float4 b, int e, int img_h, int img_w) {
    const ViewDims d = view_dims(e, img_h, img_w);
    if (e & LOFT_D4_TRANSPOSE) b = make_float4(b.y, b.x, b.w, b.z);
    if (e & LOFT_D4_MIRROR_X) { const float x1 = d.wv - b.z, x2 = d.wv - b.x; b.x = x1; b.z = x2; }
    if (e & LOFT_D4_MIRROR_Y) { const float y1 = d.hv - b.w, y2 = d.hv - b.y; b.y = y1; b.w = y2; }
    return b;
}
__device__ __forceinline__ float4 box_from_view(float4 b, int e, int img_h, int img_w) {
    const ViewDims d = view_dims(e, img_h, img_w);
    if (e & LOFT_D4_MIRROR_Y) { const float y1 = d.hv - b.w, y2 = d.hv - b.y; b.y = y1; b.w = y2; }
    if (e & LOFT_D4_MIRROR_X) { const float x1 = d.wv - b.z, x2 = d.wv - b.x; b.x = x1; b.z = x2; }
    if (e & LOFT_D4_TRANSPOSE) b = make_float4(b.y, b.x, b.w, b.z);
    return b;
}

// ---- boxes [n,4] (original frame) -> RoIs [V*n,5] view-major: bbox_mapping + bbox2roi for all views ----------------------------------
__global__ __launch_bounds__(256) void tta_view_rois_kernel(const float* __restrict__ boxes, long n, const int32_t* __restrict__ views,
                                                            int V, int img_h, int img_w, float* __restrict__ rois) {
    const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (t >= n * V) return;
    const int v = (int)(t / n);
    const long i = t - (long)v * n;
    const float4 b = box_to_view(reinterpret_cast<const float4*>(boxes)[i], views[v] & LOFT_D4_ELEMENT_MASK, img_h, img_w);
    float* o = rois + t * 5;
    o[0] = (float)v; o[1] = b.x; o[2] = b.y; o[3] = b.z; o[4] = b.w;
}
LOFT_EXPORT int loft_tta_view_rois(const float* boxes, int64_t n, const int32_t* views, int V, int img_h, int img_w, float* rois,
                                   void* stream) {
    if (V < 1 || V > TTA_MAX_VIEWS) return (int)hipErrorInvalidValue;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(tta_view_rois_kernel, dim3(loft_cdiv(n * V, 256)), dim3(256), 0, (hipStream_t)stream, boxes, (long)n, views, V,
                       img_h, img_w, rois);
    LOFT_LAUNCH_CHECK();
    return 0;
}

// ---- (props [V,P,5], counts [V]) -> compact [sum counts,5] in the original frame, scores kept ----------------------------------------
__global__ __launch_bounds__(256) void tta_gather_proposals_kernel(const float* __restrict__ props, const int64_t* __restrict__ counts,
                                                                   int V, int P, const int32_t* __restrict__ views, int img_h,
                                                                   int img_w, long out_rows, float* __restrict__ out) {
    const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (t >= (long)V * P) return;
    const int v = (int)(t / P);
    const int p = (int)(t - (long)v * P);
    long cnt = counts[v];
    cnt = cnt < 0 ? 0 : (cnt > P ? P : cnt);
    if (p >= cnt) return;
    long off = 0;
    for (int u = 0; u < v; ++u) {
        long c = counts[u];
        off += c < 0 ? 0 : (c > P ? P : c);
    }
    const long row = off + p;
    if (row >= out_rows) return;
    const float* s = props + t * 5;
    const float4 b = box_from_view(make_float4(s[0], s[1], s[2], s[3]), views[v] & LOFT_D4_ELEMENT_MASK, img_h, img_w);
    float* o = out + row * 5;
    o[0] = b.x; o[1] = b.y; o[2] = b.z; o[3] = b.w; o[4] = s[4];
}
LOFT_EXPORT int loft_tta_gather_proposals(const float* props, const int64_t* counts, int V, int P, const int32_t* views, int img_h,
                                          int img_w, int64_t out_rows, float* out, void* stream) {
    if (V < 1 || V > TTA_MAX_VIEWS) return (int)hipErrorInvalidValue;
    if (P <= 0 || out_rows <= 0) return 0;
    hipLaunchKernelGGL(tta_gather_proposals_kernel, dim3(loft_cdiv((long)V * P, 256)), dim3(256), 0, (hipStream_t)stream, props, counts,
                       V, P, views, img_h, img_w, (long)out_rows, out);
    LOFT_LAUNCH_CHECK();
    return 0;
}

// ---- aug_test_bboxes + merge_aug_bboxes: per view softmax, delta2bbox (clipped to the VIEW's shape), map back; mean over views --------
// one thread per (RoI i, column c), c = 0..C: the score of class c (c == C: background) and, for c < Cb, the box of regression class c
// (Cb = C, or 1 for a class-agnostic regressor).
__global__ __launch_bounds__(256) void tta_merge_bboxes_kernel(const float* __restrict__ rois, const float* __restrict__ bbox_pred,
                                                               const float* __restrict__ cls_score, long n, int V, int C, int Cb,
                                                               const int32_t* __restrict__ views, int img_h, int img_w, Coder4 cd,
                                                               float max_ratio, float* __restrict__ bboxes,
                                                               float* __restrict__ scores) {
    const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const int C1 = C + 1;
    if (t >= n * C1) return;
    const long i = t / C1;
    const int c = (int)(t - i * C1);
    float ssum = 0.f;
    float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int v = 0; v < V; ++v) {
        const long row = (long)v * n + i;
        const float* l = cls_score + row * C1;
        float m = l[0];
        for (int j = 1; j < C1; ++j) m = fmaxf(m, l[j]);
        float den = 0.f;
        for (int j = 0; j < C1; ++j) den += expf(l[j] - m);
        ssum += expf(l[c] - m) / den;
        if (c < Cb) {
            const int e = views[v] & LOFT_D4_ELEMENT_MASK;
            const ViewDims d = view_dims(e, img_h, img_w);
            const float* r = rois + row * 5;
            const float4 dl = reinterpret_cast<const float4*>(bbox_pred)[row * Cb + c];
            const float4 bv = decode_box(make_float4(r[1], r[2], r[3], r[4]), dl.x, dl.y, dl.z, dl.w, cd.means, cd.stds, max_ratio, d.hv,
                                         d.wv);
            const float4 b = box_from_view(bv, e, img_h, img_w);
            bsum.x += b.x; bsum.y += b.y; bsum.z += b.z; bsum.w += b.w;
        }
    }
    const float fv = (float)V;
    scores[t] = ssum / fv;
    if (c < Cb) reinterpret_cast<float4*>(bboxes)[i * Cb + c] = make_float4(bsum.x / fv, bsum.y / fv, bsum.z / fv, bsum.w / fv);
}
LOFT_EXPORT int loft_tta_merge_bboxes(const float* rois, const float* bbox_pred, const float* cls_score, int64_t n, int V, int C, int Cb,
                                      const int32_t* views, int img_h, int img_w, const float* means_host, const float* stds_host,
                                      float wh_ratio_clip, float* bboxes, float* scores, void* stream) {
    if (V < 1 || V > TTA_MAX_VIEWS || C < 1 || (Cb != C && Cb != 1)) return (int)hipErrorInvalidValue;
    if (n <= 0) return 0;
    Coder4 cd;
    for (int i = 0; i < 4; ++i) { cd.means[i] = means_host[i]; cd.stds[i] = stds_host[i]; }
    const float max_ratio = fabsf(logf(wh_ratio_clip));
    hipLaunchKernelGGL(tta_merge_bboxes_kernel, dim3(loft_cdiv(n * (C + 1), 256)), dim3(256), 0, (hipStream_t)stream, rois, bbox_pred,
                       cls_score, (long)n, V, C, Cb, views, img_h, img_w, cd, max_ratio, bboxes, scores);
    LOFT_LAUNCH_CHECK();
    return 0;
}

// ---- merged offsets (an extension: the reference's aug_test returns none) -------------------------------------------------------------
// pred: what ONE run of the offset head over the view-major RoIs [V*n,5] returns -- FOA (reg_num == 0) [4, V*n, 2] branch-major, or
// the plain head's [V*n, reg_num]; rois: those RoIs, i.e. the view boxes.
// Per view the decode of the single-view path (box_codec.h), the vector mapped back by the inverse element; mean over views.
__global__ __launch_bounds__(256) void tta_merge_offsets_kernel(const float* __restrict__ pred, const float* __restrict__ rois, long n,
                                                                int V, int reg_num, const int32_t* __restrict__ views, float mean_x,
                                                                float mean_y, float std_x, float std_y, float max_h, float max_w,
                                                                int polar, float* __restrict__ out) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    float sx = 0.f, sy = 0.f;
    for (int v = 0; v < V; ++v) {
        const int e = views[v] & LOFT_D4_ELEMENT_MASK;
        const float* r = rois + ((long)v * n + i) * 5;
        const float4 b = make_float4(r[1], r[2], r[3], r[4]);
        // the clamp bounds belong to the view's axes
        const float mh = (e & LOFT_D4_TRANSPOSE) ? max_w : max_h, mw = (e & LOFT_D4_TRANSPOSE) ? max_h : max_w;
        float2 g;
        if (reg_num == 0) g = foa_fuse_decode_one(pred, (long)V * n, (long)v * n + i, b, std_x, std_y, mh, mw);
        else g = offset_decode_one(pred, (long)v * n + i, b, mean_x, mean_y, std_x, std_y, mh, mw, reg_num, polar);
        if (e & LOFT_D4_MIRROR_Y) g.y = -g.y;
        if (e & LOFT_D4_MIRROR_X) g.x = -g.x;
        if (e & LOFT_D4_TRANSPOSE) g = make_float2(g.y, g.x);
        sx += g.x; sy += g.y;
    }
    out[2 * i] = sx / (float)V; out[2 * i + 1] = sy / (float)V;
}
LOFT_EXPORT int loft_tta_merge_offsets(const float* pred, const float* rois, int64_t n, int V, int reg_num, const int32_t* views,
                                       float mean_x, float mean_y, float std_x, float std_y, float max_h, float max_w, int polar,
                                       float* out, void* stream) {
    if (V < 1 || V > TTA_MAX_VIEWS || (reg_num != 0 && reg_num != 2 && reg_num != 3)) return (int)hipErrorInvalidValue;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(tta_merge_offsets_kernel, dim3(loft_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, pred, rois, (long)n, V,
                       reg_num, views, mean_x, mean_y, std_x, std_y, max_h, max_w, polar, out);
    LOFT_LAUNCH_CHECK();
    return 0;
}

// ---- aug_test_mask + merge_aug_masks + the paste, in one launch ----------------------------------------------------------------------
// logits fp32 [V,N,S,S] (class selected), boxes [N,4] in the original frame -> uint8 {0,1} [N,img_h,img_w].  One workgroup per
// (detection, band of PASTE_ROWS image rows).  A band the box's tight region does not reach is zero-filled with 16-byte stores and
// reads nothing else.  Otherwise the workgroup first stages the detection's merged taps in LDS -- tap (r, c) = mean over views of
// sigmoid(logit) read through the view's inverse permutation of the grid; the merged probabilities exist nowhere else -- and then
// every thread produces 16 pixels of a row per step: bilinear rule, tight integer region and threshold are mask_paste_kernel's
// (box_codec.h), packed into one 16-byte store.  (mask_paste_kernel launches a thread per pixel per detection, most of which write
// one zero byte.)  A width that is no multiple of 16 takes byte stores.
#define PASTE_ROWS 16
#define PASTE_MAX_S 64
__global__ __launch_bounds__(256) void mask_paste_views_kernel(const float* __restrict__ logits, const float* __restrict__ boxes, int N,
                                                               int V, int S, const int32_t* __restrict__ views, int img_h, int img_w,
                                                               float thr, uint8_t* __restrict__ out) {
    __shared__ float taps[PASTE_MAX_S * PASTE_MAX_S];
    const int n = blockIdx.y;
    const int y_lo = blockIdx.x * PASTE_ROWS;
    const int y_hi = min(y_lo + PASTE_ROWS, img_h);
    const float4 b = reinterpret_cast<const float4*>(boxes)[n];
    uint8_t* o = out + (long)n * img_h * img_w;
    const bool wide = (img_w & 15) == 0;
    // (workgroup-uniform) rows of this band inside the box's tight region?
    const float ry0 = fmaxf(floorf(b.y) - 1.f, 0.f), ry1 = fminf(ceilf(b.w) + 1.f, (float)img_h);
    const bool touched = (float)(y_hi - 1) >= ry0 && (float)y_lo < ry1;
    if (!touched) {
        if (wide) {
            const int per_row = img_w >> 4, total = (y_hi - y_lo) * per_row;
            uint4* dst = reinterpret_cast<uint4*>(o + (long)y_lo * img_w);      // band rows are contiguous
            for (int k = threadIdx.x; k < total; k += blockDim.x) dst[k] = make_uint4(0u, 0u, 0u, 0u);
        } else {
            const int total = (y_hi - y_lo) * img_w;
            for (int k = threadIdx.x; k < total; k += blockDim.x) o[(long)y_lo * img_w + k] = 0;
        }
        return;
    }
    paste_stage_taps(taps, logits, n, N, V, S, views);
    __syncthreads();
    auto at = [&](int yy, int xx) -> float {
        if (yy < 0 || yy >= S || xx < 0 || xx >= S) return 0.f;
        return taps[yy * S + xx];
    };
    if (wide) {
        const int per_row = img_w >> 4, total = (y_hi - y_lo) * per_row;
        const float rx0 = fmaxf(floorf(b.x) - 1.f, 0.f), rx1 = fminf(ceilf(b.z) + 1.f, (float)img_w);
        for (int k = threadIdx.x; k < total; k += blockDim.x) {
            const int y = y_lo + k / per_row, x0 = (k % per_row) << 4;
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            if ((float)(x0 + 15) >= rx0 && (float)x0 < rx1 && (float)y >= ry0 && (float)y < ry1) {
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int x = x0 + j;
                    if (paste_outside(x, y, b, img_h, img_w)) continue;
                    if (paste_sample(x, y, b, S, at) >= thr) w[j >> 2] |= 1u << ((j & 3) * 8);
                }
            }
            reinterpret_cast<uint4*>(o + (long)y * img_w)[x0 >> 4] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    } else {
        const int total = (y_hi - y_lo) * img_w;
        for (int k = threadIdx.x; k < total; k += blockDim.x) {
            const int y = y_lo + k / img_w, x = k % img_w;
            uint8_t bit = 0;
            if (!paste_outside(x, y, b, img_h, img_w)) bit = paste_sample(x, y, b, S, at) >= thr ? 1 : 0;
            o[(long)y * img_w + x] = bit;
        }
    }
}
LOFT_EXPORT int loft_mask_paste_views(const float* logits, const float* boxes, int N, int V, int S, const int32_t* views, int img_h,
                                      int img_w, float thr, uint8_t* out, void* stream) {
    if (V < 1 || V > TTA_MAX_VIEWS || S < 1 || S > PASTE_MAX_S || img_h < 1 || img_w < 1) return (int)hipErrorInvalidValue;
    if (N <= 0) return 0;
    if (N > 65535) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(mask_paste_views_kernel, dim3(loft_cdiv(img_h, PASTE_ROWS), N), dim3(256), 0, (hipStream_t)stream, logits, boxes,
                       N, V, S, views, img_h, img_w, thr, out);
    LOFT_LAUNCH_CHECK();
    return 0;
}
