// eval_pairs.hip -- the pixel counts the BONAI metric pairs buildings on (bonai_amd/evaluation.py), one launch per image.
// gfx950 only.
//
// tools/bonai/bonai_evaluation.py:461-475 pairs every prediction with every ground-truth building whose
// iou = inter / (area_pred + area_gt - inter + 1) reaches 0.5.  On bitmaps that is, per image, a [P, G] matrix of pixel
// intersections and the P + G areas.  evaluation._intersections takes them with one slice + AND + sum + read-back per prediction;
// here one launch writes all of them:
//   * blocks [0, P * ceil(G / 32)): prediction p against a chunk of 32 ground truths.  The prediction's window (clipped to the
//     image, widened to 16-byte units, bytes outside the window zeroed) is staged ONCE per workgroup into LDS, in strips of rows
//     that fit 32 KiB; each of the 4 waves then owns 8 ground truths of the chunk and walks their rows in 16-byte units along x
//     (lane = consecutive unit), AND + v_sad_u8 byte sums into one 32-bit accumulator per lane and ground truth.  With ``gbox``
//     the walk is restricted to window x gbox[g], and skipped when that is empty: a ground truth's set pixels all lie inside
//     its gbox, so every pixel left out contributes 0 and the counts are the same with, without, or with a looser gbox.
//   * blocks after those: one per mask, its full-image byte sum (area_p, area_g).
// No atomics: every output element has exactly one writer (lane 0 of one wave after a shuffle reduction of integers), so the
// results are exact and the same from run to run.  The largest count, H * W = 2^20 at tile size, is far inside 32 bits, and no
// partial sum is narrower than that.
// 16-byte global accesses need W % 16 == 0 and 16-byte aligned bases (``vec``); any other geometry takes the same code with the
// unit assembled from guarded byte loads.
#include "loft_common.h"

#define PAIR_THREADS 256
#define PAIR_WAVES 4
#define PAIR_GCHUNK 32
#define PAIR_GPW (PAIR_GCHUNK / PAIR_WAVES)
#define PAIR_TILE_UNITS 2048          /* 16-byte units of LDS per strip (32 KiB) */

// 16 mask bytes of one row starting at x (x % 16 == 0, 0 <= x < W); bytes at or past W read as 0
__device__ __forceinline__ uint4 pair_load_unit(const uint8_t* __restrict__ row, int x, int W, bool vec) {
    if (vec) return *reinterpret_cast<const uint4*>(row + x);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (x + i < W) w[i >> 2] |= (uint32_t)row[x + i] << (8 * (i & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// acc + the sum of the 16 bytes of (a & b)
__device__ __forceinline__ uint32_t pair_and_sum(const uint4 a, const uint4 b, uint32_t acc) {
    acc = __builtin_amdgcn_sad_u8(a.x & b.x, 0u, acc);
    acc = __builtin_amdgcn_sad_u8(a.y & b.y, 0u, acc);
    acc = __builtin_amdgcn_sad_u8(a.z & b.z, 0u, acc);
    return __builtin_amdgcn_sad_u8(a.w & b.w, 0u, acc);
}

__device__ __forceinline__ uint32_t pair_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__global__ __launch_bounds__(PAIR_THREADS) void mask_pair_counts_kernel(
        const uint8_t* __restrict__ pm, const uint8_t* __restrict__ gm, const int* __restrict__ win, const int* __restrict__ gbox,
        int P, int G, int H, int W, int vec_, int* __restrict__ inter, int* __restrict__ area_p, int* __restrict__ area_g) {
    __shared__ uint4 tile[PAIR_TILE_UNITS];
    __shared__ uint32_t part[PAIR_WAVES];
    const bool vec = vec_ != 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gchunks = (G + PAIR_GCHUNK - 1) / PAIR_GCHUNK;
    int b = blockIdx.x;
    const size_t plane = (size_t)H * W;

    if (b >= P * gchunks) {                                  // ---- area of one mask
        b -= P * gchunks;
        const uint8_t* m = b < P ? pm + (size_t)b * plane : gm + (size_t)(b - P) * plane;
        uint32_t s = 0;
        if (vec) {                                           // (W % 16 == 0: the plane is a whole number of units)
            const uint4* q = reinterpret_cast<const uint4*>(m);
            const uint4 ones = make_uint4(~0u, ~0u, ~0u, ~0u);
            for (size_t i = threadIdx.x; i < plane / 16; i += PAIR_THREADS) s = pair_and_sum(q[i], ones, s);
        } else {
            for (size_t i = threadIdx.x; i < plane; i += PAIR_THREADS) s += m[i];
        }
        s = pair_wave_sum(s);
        if (lane == 0) part[wave] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int a = (int)(part[0] + part[1] + part[2] + part[3]);
            if (b < P) area_p[b] = a; else area_g[b - P] = a;
        }
        return;
    }

    // ---- prediction p against ground truths [g0, g0 + 32)
    const int p = b / gchunks, g0 = (b - p * gchunks) * PAIR_GCHUNK;
    const int x0 = max(win[4 * p], 0), y0 = max(win[4 * p + 1], 0), x1 = min(win[4 * p + 2], W), y1 = min(win[4 * p + 3], H);
    uint32_t acc[PAIR_GPW];
#pragma unroll
    for (int k = 0; k < PAIR_GPW; ++k) acc[k] = 0;
    if (x1 > x0 && y1 > y0) {                                // (block-uniform: the barriers below are reached by all or none)
        const int xa = x0 & ~15;
        const int nu = ((x1 + 15) >> 4) - (xa >> 4);         // units per window row; <= PAIR_TILE_UNITS (checked by the host)
        const int srows = PAIR_TILE_UNITS / nu;
        const uint8_t* pbase = pm + (size_t)p * plane;
        for (int ys = y0; ys < y1; ys += srows) {
            const int ye = min(ys + srows, y1);
            const int n = (ye - ys) * nu;
            __syncthreads();                                 // the previous strip has been read by every wave
            for (int i = threadIdx.x; i < n; i += PAIR_THREADS) {
                const int r = i / nu, x = xa + 16 * (i - r * nu);
                const uint4 v = pair_load_unit(pbase + (size_t)(ys + r) * W, x, W, vec);
                uint32_t w[4] = {v.x, v.y, v.z, v.w};
                if (x < x0 || x + 16 > x1) {                 // an edge unit: bytes outside [x0, x1) do not count
#pragma unroll
                    for (int j = 0; j < 16; ++j)
                        if (x + j < x0 || x + j >= x1) w[j >> 2] &= ~(0xffu << (8 * (j & 3)));
                }
                tile[i] = make_uint4(w[0], w[1], w[2], w[3]);
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < PAIR_GPW; ++k) {
                const int g = g0 + k * PAIR_WAVES + wave;    // (wave-uniform)
                if (g >= G) continue;
                int cx0 = x0, cy0 = ys, cx1 = x1, cy1 = ye;
                if (gbox != nullptr) {
                    cx0 = max(cx0, gbox[4 * g]); cy0 = max(cy0, gbox[4 * g + 1]);
                    cx1 = min(cx1, gbox[4 * g + 2]); cy1 = min(cy1, gbox[4 * g + 3]);
                }
                if (cx1 <= cx0 || cy1 <= cy0) continue;
                const int ua = (cx0 - xa) >> 4, cu = ((cx1 - xa + 15) >> 4) - ua;
                const int m = (cy1 - cy0) * cu;
                const uint8_t* gb = gm + (size_t)g * plane;
                uint32_t s = acc[k];
                for (int i = lane; i < m; i += 64) {
                    const int r = i / cu, u = ua + (i - r * cu), y = cy0 + r;
                    s = pair_and_sum(tile[(y - ys) * nu + u], pair_load_unit(gb + (size_t)y * W, xa + 16 * u, W, vec), s);
                }
                acc[k] = s;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < PAIR_GPW; ++k) {
        const int g = g0 + k * PAIR_WAVES + wave;
        if (g >= G) continue;
        const uint32_t s = pair_wave_sum(acc[k]);
        if (lane == 0) inter[(size_t)p * G + g] = (int)s;
    }
}

LOFT_EXPORT int loft_mask_pair_counts_u8(const uint8_t* pm, const uint8_t* gm, const int* win, const int* gbox, int P, int G,
                                         int H, int W, int* inter, int* area_p, int* area_g, void* stream) {
    if (P < 0 || G < 0 || H <= 0 || W <= 0) return (int)hipErrorInvalidValue;
    if (P == 0 || G == 0) return 0;
    if ((W + 15) / 16 + 1 > PAIR_TILE_UNITS || (long)H * W >= (1L << 31)) return (int)hipErrorInvalidValue;
    const long blocks = (long)P * loft_cdiv(G, PAIR_GCHUNK) + P + G;
    if (blocks >= (1L << 31)) return (int)hipErrorInvalidValue;
    const int vec = (W % 16 == 0) && (((uintptr_t)pm | (uintptr_t)gm) & 15) == 0;
    hipLaunchKernelGGL(mask_pair_counts_kernel, dim3((unsigned)blocks), dim3(PAIR_THREADS), 0, (hipStream_t)stream, pm, gm, win,
                       gbox, P, G, H, W, vec, inter, area_p, area_g);
    LOFT_LAUNCH_CHECK();
    return 0;
}
