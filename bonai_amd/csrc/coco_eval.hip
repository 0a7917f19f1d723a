// coco_eval.hip -- COCOeval on the device: IoU with crowd semantics, the greedy per-threshold matching of evaluateImg and the
// precision / recall accumulation of accumulate (cocoapi PythonAPI/pycocotools/cocoeval.py and common/maskApi.c, restated from the
// published source; pycocotools is not in the tree and nothing here has been run against it).  gfx950 only.
//
// Everything that decides a result is fp64 or integer, and the file is compiled with -ffp-contract=off: a quotient here is the
// IEEE quotient numpy / C compute from the same operands, so the outputs are exact, not approximate.
//   * coco_iou_kernel: one thread per (detection, ground truth) pair.  Boxes: bbIou (no "+1"; 0 when the boxes do not overlap).
//     Masks: rleIou from the pixel counts of loft_mask_pair_counts_u8 (0 when the intersection is empty).  A crowd ground truth
//     divides by the detection's area alone.  Neither form can produce a NaN.
//   * coco_match_kernel: one workgroup per (segment, area range), one wave per IoU threshold.  Wave 0 first lays the segment's
//     ground truths out in the order evaluateImg visits them (argsort(gtIg, kind='mergesort'): non-ignored first, then ignored,
//     each group in input order) with two ballot passes; every wave then walks the detections in order and takes a wave-wide
//     arg-max over the ground truths, 64 per step.  evaluateImg's scan "skip iou < bound, else take and raise the bound" is a
//     maximum whose ties go to the LAST ground truth visited; "stop at the first ignored ground truth once a non-ignored match is
//     held" makes it a maximum over the non-ignored group and, only when that group gives nothing, over the ignored group.  A
//     wave's matched flags are bits in LDS that only that wave reads and writes.
//   * coco_pack_kernel: one thread per detection folds its A*T (matched, ignored) results into two 64-bit words.
//   * coco_accumulate_kernel: one workgroup per (threshold, area range, max-detections) walks the globally score-sorted records
//     alone -- no workgroup waits on another.  Running tp / fp counts are integers (ballot prefix sums); each counted detection
//     raises the bucket of the largest recall threshold its recall satisfies (LDS atomic max on the bit pattern: non-negative
//     doubles order as their bit patterns), and a suffix maximum over the buckets is accumulate's right-to-left envelope followed
//     by searchsorted(rc, recThrs, 'left').
#include "loft_common.h"

#define COCO_MAX_GT 4096            /* LOFT_COCO_MAX_GT */
#define COCO_MAX_T 16               /* LOFT_COCO_MAX_THRS */
#define COCO_MAX_R 128              /* LOFT_COCO_MAX_RECS */
#define COCO_TOO_MANY_GT (-2)       /* LOFT_COCO_TOO_MANY_GT */
#define COCO_IG (1u << 30)
#define COCO_CROWD (1u << 31)
#define COCO_IDX 0xffffu
#define COCO_ACC_THREADS 256

// ---- IoU -------------------------------------------------------------------------------------------------------------------
template <bool MASK>
__global__ __launch_bounds__(256) void coco_iou_kernel(const double* __restrict__ dt, const double* __restrict__ gt,
                                                       const int* __restrict__ inter, const int* __restrict__ area_p,
                                                       const int* __restrict__ area_g, const uint8_t* __restrict__ iscrowd,
                                                       int D, int G, double* __restrict__ out) {
    const int64_t n = (int64_t)D * G;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) {
        const int d = (int)(k / G), g = (int)(k - (int64_t)d * G);
        const bool crowd = iscrowd[g] != 0;
        double o = 0.0;
        if (MASK) {
            const int i = inter[k];
            if (i != 0) {
                const double u = crowd ? (double)area_p[d] : (double)area_p[d] + (double)area_g[g] - (double)i;
                o = (double)i / u;
            }
        } else {
            const double* a = dt + 4 * (int64_t)d;
            const double* b = gt + 4 * (int64_t)g;
            const double da = a[2] * a[3], ga = b[2] * b[3];
            const double w = fmin(a[2] + a[0], b[2] + b[0]) - fmax(a[0], b[0]);
            const double h = fmin(a[3] + a[1], b[3] + b[1]) - fmax(a[1], b[1]);
            if (w > 0 && h > 0) {
                const double i = w * h;
                const double u = crowd ? da : da + ga - i;
                o = i / u;
            }
        }
        out[k] = o;
    }
}

static int coco_iou_grid(int64_t n) { return (int)((n + 255) / 256 < 65536 ? (n + 255) / 256 : 65536); }

LOFT_EXPORT int loft_coco_box_iou(const double* dt, const double* gt, const uint8_t* iscrowd, int D, int G, double* out,
                                  void* stream) {
    if (D < 0 || G < 0) return (int)hipErrorInvalidValue;
    if (D == 0 || G == 0) return 0;
    hipLaunchKernelGGL(coco_iou_kernel<false>, dim3(coco_iou_grid((int64_t)D * G)), dim3(256), 0, (hipStream_t)stream, dt, gt,
                       (const int*)nullptr, (const int*)nullptr, (const int*)nullptr, iscrowd, D, G, out);
    LOFT_LAUNCH_CHECK();
    return 0;
}

LOFT_EXPORT int loft_coco_mask_iou(const int* inter, const int* area_p, const int* area_g, const uint8_t* iscrowd, int D, int G,
                                   double* out, void* stream) {
    if (D < 0 || G < 0) return (int)hipErrorInvalidValue;
    if (D == 0 || G == 0) return 0;
    hipLaunchKernelGGL(coco_iou_kernel<true>, dim3(coco_iou_grid((int64_t)D * G)), dim3(256), 0, (hipStream_t)stream,
                       (const double*)nullptr, (const double*)nullptr, inter, area_p, area_g, iscrowd, D, G, out);
    LOFT_LAUNCH_CHECK();
    return 0;
}

// ---- matching --------------------------------------------------------------------------------------------------------------
// (value, position) of the better of two candidates: the larger IoU, and among equals the later position.  A lane without a
// candidate carries (bound, -1): it loses every tie.
__device__ __forceinline__ void coco_wave_argmax(double& v, int& p) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const double v2 = __shfl_xor(v, o, 64);
        const int p2 = __shfl_xor(p, o, 64);
        if (v2 > v || (v2 == v && p2 > p)) { v = v2; p = p2; }
    }
}

__global__ __launch_bounds__(64 * COCO_MAX_T) void coco_match_kernel(
        const double* __restrict__ ious, const int64_t* __restrict__ iou_off, const int64_t* __restrict__ det_off,
        const int64_t* __restrict__ gt_off, const double* __restrict__ det_area, const double* __restrict__ gt_area,
        const uint8_t* __restrict__ gt_crowd, const double* __restrict__ thrs, const double* __restrict__ area_rng, int T, int A,
        int* __restrict__ gt_match, uint8_t* __restrict__ det_ign, int* __restrict__ npig) {
    __shared__ uint32_t order[COCO_MAX_GT];                  // visiting order: ground-truth index | COCO_IG | COCO_CROWD
    __shared__ uint32_t gtm_all[COCO_MAX_T][COCO_MAX_GT / 32];
    __shared__ int s_np;
    const int s = blockIdx.x / A, a = blockIdx.x - s * A;
    const int lane = threadIdx.x & 63, t = threadIdx.x >> 6;                 // (t < T: the block has exactly T waves)
    const int64_t d0 = det_off[s], g0 = gt_off[s];
    const int D = (int)(det_off[s + 1] - d0), G = (int)(gt_off[s + 1] - g0); // G <= COCO_MAX_GT (checked by the host)
    const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
    volatile uint32_t* gtm = gtm_all[t];
    for (int i = lane; i < (G + 31) / 32; i += 64) gtm[i] = 0u;
    if (t == 0) {
        const uint64_t below = (1ull << lane) - 1ull;
        int np = 0;
        for (int c = 0; c < G; c += 64) {
            const int g = c + lane;
            const bool keep = g < G && !(gt_crowd[g0 + g] != 0 || gt_area[g0 + g] < lo || gt_area[g0 + g] > hi);
            np += __popcll(__ballot(keep));
        }
        int run_n = 0, run_i = np;
        for (int c = 0; c < G; c += 64) {
            const int g = c + lane;
            const bool valid = g < G;
            const bool crowd = valid && gt_crowd[g0 + g] != 0;
            const bool ig = valid && (crowd || gt_area[g0 + g] < lo || gt_area[g0 + g] > hi);
            const uint64_t mn = __ballot(valid && !ig), mi = __ballot(ig);
            if (valid) {
                const int pos = ig ? run_i + __popcll(mi & below) : run_n + __popcll(mn & below);   // a permutation of [0, G)
                order[pos] = (uint32_t)g | (ig ? COCO_IG : 0u) | (crowd ? COCO_CROWD : 0u);
            }
            run_n += __popcll(mn);
            run_i += __popcll(mi);
        }
        if (lane == 0) { s_np = np; npig[s * A + a] = np; }
    }
    __syncthreads();
    const int np = s_np;
    const double thr = fmin(thrs[t], 1.0 - 1e-10);
    const int AT = A * T, slot = a * T + t;
    const double* base = ious + iou_off[s];
    for (int d = 0; d < D; ++d) {
        const double* row = base + (int64_t)d * G;
        double v = thr;
        int p = -1;
        for (int pos = lane; pos < np; pos += 64) {                          // the non-ignored group: no crowds in it
            if ((gtm[pos >> 5] >> (pos & 31)) & 1u) continue;
            const double x = row[order[pos] & COCO_IDX];
            if (!(x < v)) { v = x; p = pos; }
        }
        coco_wave_argmax(v, p);
        if (p < 0) {                                                         // (wave-uniform after the reduction)
            for (int pos = np + lane; pos < G; pos += 64) {                  // the ignored group: a matched crowd stays open
                const uint32_t e = order[pos];
                if (((gtm[pos >> 5] >> (pos & 31)) & 1u) && !(e & COCO_CROWD)) continue;
                const double x = row[e & COCO_IDX];
                if (!(x < v)) { v = x; p = pos; }
            }
            coco_wave_argmax(v, p);
        }
        if (lane == 0) {
            const int64_t o = (d0 + d) * AT + slot;
            if (p >= 0) {
                const uint32_t e = order[p];
                gtm[p >> 5] |= 1u << (p & 31);
                gt_match[o] = (int)(e & COCO_IDX);
                det_ign[o] = (e & COCO_IG) ? 1 : 0;
            } else {
                const double da = det_area[d0 + d];
                gt_match[o] = -1;
                det_ign[o] = (da < lo || da > hi) ? 1 : 0;
            }
        }
        __builtin_amdgcn_wave_barrier();                                     // (the flag is read by the other lanes next round)
    }
}

__global__ __launch_bounds__(256) void coco_pack_kernel(const int* __restrict__ gt_match, const uint8_t* __restrict__ det_ign,
                                                        int64_t N, int AT, uint64_t* __restrict__ bits) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    uint64_t m = 0, ig = 0;
    for (int k = 0; k < AT; ++k) {
        if (gt_match[n * AT + k] >= 0) m |= 1ull << k;
        if (det_ign[n * AT + k]) ig |= 1ull << k;
    }
    bits[2 * n] = m;
    bits[2 * n + 1] = ig;
}

LOFT_EXPORT int loft_coco_match(const double* ious, const int64_t* iou_off, const int64_t* det_off, const int64_t* gt_off,
                                const double* det_area, const double* gt_area, const uint8_t* gt_crowd, const double* thrs,
                                const double* area_rng, int S, int64_t total_det, int max_gt, int T, int A, int32_t* gt_match,
                                uint8_t* det_ign, uint64_t* bits, int32_t* npig, void* stream) {
    if (S < 0 || total_det < 0 || max_gt < 0 || T < 1 || T > COCO_MAX_T || A < 1 || A * T > 64) return (int)hipErrorInvalidValue;
    if (max_gt > COCO_MAX_GT) return COCO_TOO_MANY_GT;
    if ((int64_t)S * A >= (1ll << 31) || (total_det + 255) / 256 >= (1ll << 31)) return (int)hipErrorInvalidValue;
    if (S == 0) return 0;
    hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)(S * A)), dim3(64 * T), 0, (hipStream_t)stream, ious, iou_off, det_off,
                       gt_off, det_area, gt_area, gt_crowd, thrs, area_rng, T, A, gt_match, det_ign, npig);
    LOFT_LAUNCH_CHECK();
    if (total_det > 0) {
        hipLaunchKernelGGL(coco_pack_kernel, dim3((unsigned)((total_det + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           (const int*)gt_match, (const uint8_t*)det_ign, total_det, A * T, bits);
        LOFT_LAUNCH_CHECK();
    }
    return 0;
}

// ---- accumulation ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(COCO_ACC_THREADS) void coco_accumulate_kernel(
        const uint64_t* __restrict__ bits, const int* __restrict__ rank, const int* __restrict__ perm, int64_t N,
        const int64_t* __restrict__ npig, const int* __restrict__ max_dets, const double* __restrict__ rec_thrs, int T, int A, int M,
        int R, double* __restrict__ precision, double* __restrict__ recall) {
    __shared__ unsigned long long bucket[COCO_MAX_R];
    __shared__ double rthr[COCO_MAX_R];
    __shared__ int wsum[2][COCO_ACC_THREADS / 64][2];
    const int m = blockIdx.x % M, a = (blockIdx.x / M) % A, t = blockIdx.x / (M * A);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t np = npig[a];
    if (np == 0) {                                                           // (block-uniform) both stay -1
        for (int r = tid; r < R; r += COCO_ACC_THREADS) precision[(((int64_t)t * R + r) * A + a) * M + m] = -1.0;
        if (tid == 0) recall[((int64_t)t * A + a) * M + m] = -1.0;
        return;
    }
    for (int r = tid; r < R; r += COCO_ACC_THREADS) { bucket[r] = 0ull; rthr[r] = rec_thrs[r]; }
    __syncthreads();
    const int md = max_dets[m], slot = a * T + t;
    const double npd = (double)np;
    const uint64_t upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;
    int64_t tp_run = 0, fp_run = 0, nd = 0;
    int buf = 0;
    for (int64_t c = 0; c < N; c += COCO_ACC_THREADS, buf ^= 1) {
        const int64_t i = c + tid;
        bool counted = false, tpf = false, fpf = false;
        if (i < N) {
            const int j = perm[i];
            if (rank[j] < md) {
                const bool mt = (bits[2 * (int64_t)j] >> slot) & 1ull, ig = (bits[2 * (int64_t)j + 1] >> slot) & 1ull;
                counted = true;
                tpf = mt && !ig;
                fpf = !mt && !ig;
            }
        }
        const uint64_t bt = __ballot(tpf), bf = __ballot(fpf);
        if (lane == 0) { wsum[buf][wave][0] = __popcll(bt); wsum[buf][wave][1] = __popcll(bf); }
        nd += __syncthreads_count(counted);                                  // (the other buffer is free: one barrier per chunk)
        int64_t tp = tp_run + __popcll(bt & upto), fp = fp_run + __popcll(bf & upto);
#pragma unroll
        for (int w = 0; w < COCO_ACC_THREADS / 64; ++w) {
            if (w < wave) { tp += wsum[buf][w][0]; fp += wsum[buf][w][1]; }
            tp_run += wsum[buf][w][0];
            fp_run += wsum[buf][w][1];
        }
        if (counted) {
            const double rc = (double)tp / npd;
            const double pr = (double)tp / (((double)fp + (double)tp) + 0x1p-52);           // np.spacing(1)
            int lo_ = 0, hi_ = R;                                            // number of thresholds <= rc
            while (lo_ < hi_) {
                const int mid = (lo_ + hi_) >> 1;
                if (rthr[mid] <= rc) lo_ = mid + 1; else hi_ = mid;
            }
            if (lo_ > 0) atomicMax(&bucket[lo_ - 1], (unsigned long long)__double_as_longlong(pr));
        }
    }
    __syncthreads();
    for (int r = tid; r < R; r += COCO_ACC_THREADS) {
        unsigned long long best = 0ull;
        for (int b = r; b < R; ++b) best = bucket[b] > best ? bucket[b] : best;
        precision[(((int64_t)t * R + r) * A + a) * M + m] = __longlong_as_double((long long)best);
    }
    if (tid == 0) recall[((int64_t)t * A + a) * M + m] = nd ? (double)tp_run / npd : 0.0;
}

LOFT_EXPORT int loft_coco_accumulate(const uint64_t* bits, const int32_t* rank, const int32_t* perm, int64_t N, const int64_t* npig,
                                     const int32_t* max_dets, const double* rec_thrs, int T, int A, int M, int R, double* precision,
                                     double* recall, void* stream) {
    if (N < 0 || N >= (1ll << 31) || T < 1 || A < 1 || A * T > 64 || M < 1 || R < 1 || R > COCO_MAX_R) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(coco_accumulate_kernel, dim3((unsigned)(T * A * M)), dim3(COCO_ACC_THREADS), 0, (hipStream_t)stream, bits,
                       (const int*)rank, (const int*)perm, N, npig, (const int*)max_dets, rec_thrs, T, A, M, R, precision, recall);
    LOFT_LAUNCH_CHECK();
    return 0;
}
