// scene.hip -- whole-scene inference (bonai_amd/scene.py): overlapping tiles cut out of ONE uploaded uint8 image, and the merge of
// the tiles' detections on their MASKS.  An extension: the reference's tools/bonai/bonai_test.py hands the merge to an external
// package, so there is nothing to mirror; the rule is stated here and in the README.
//
//   loft_scene_tile_prep     uint8 scene [H,W,3] + a device table of tile origins -> normalised fp32 tiles [n,3,th,tw], zero where a
//                            tile leaves the scene (the reference's Pad after Normalize).  The per-pixel statement is image_prep.h's,
//                            the one loft_image_prep_d4 stores with.
//   loft_scene_pair_counts   the mask of detection i is BY DEFINITION the paste of its logits at its scene-frame box on the H x W
//                            canvas (box_codec.h: paste_stage_taps, paste_outside, paste_sample >= thr) -- what loft_mask_paste
//                            writes and loft_mask_rle encodes.  area[i] and, for every pair of detections of DIFFERENT tiles whose
//                            integer paste windows intersect, a record (i, j, |mask_i & mask_j|), i < j.  No canvas, no bitmaps,
//                            no N x N table: only window pixels are evaluated, from the S x S taps in LDS.
//   loft_scene_suppress      greedy suppression in priority order over the records' edges, as rounds to a fixed point.
// Built with -ffp-contract=off (box_codec.h: the same pixels as boxes.hip / mask_rle.hip set).
#include "loft_common.h"
#include "box_codec.h"
#include "image_prep.h"
#include "../../include/loft_hip.h"

// ---- tiles of a scene -------------------------------------------------------------------------------------------------------------
// One workgroup per 64 x 64 block of one output tile.  The block's source rows start at any byte of the scene (an origin is any
// pixel, a pixel three bytes), so a row segment is copied into LDS as the aligned dwords that cover it and read back at its byte
// shift: global reads and global writes both run along rows.  194 bytes at most (64 pixels + 3 of shift - 1) = 49 dwords, an odd
// pitch.
#define SC_TILE 64
#define SC_PITCH 49

__global__ __launch_bounds__(256) void scene_tile_prep_kernel(const uint8_t* __restrict__ scene, int H, int W,
                                                              const int32_t* __restrict__ origins, int th, int tw, int keep,
                                                              PrepNorm nm, float* __restrict__ out) {
    __shared__ unsigned tile[SC_TILE * SC_PITCH];
    const int n = blockIdx.z, tx0 = blockIdx.x * SC_TILE, ty0 = blockIdx.y * SC_TILE;
    const int cw = min(SC_TILE, tw - tx0), ch = min(SC_TILE, th - ty0);
    const long long sx0 = (long long)origins[2 * n] + tx0, sy0 = (long long)origins[2 * n + 1] + ty0;   // the block's first pixel
    // the block's columns [c_lo, c_hi) and rows [r_lo, r_hi) that lie inside the scene (whatever the table holds)
    const int c_lo = (int)min(max(-sx0, 0ll), (long long)cw), c_hi = (int)min(max((long long)W - sx0, (long long)c_lo), (long long)cw);
    const int r_lo = (int)min(max(-sy0, 0ll), (long long)ch), r_hi = (int)min(max((long long)H - sy0, (long long)r_lo), (long long)ch);
    const long long total = (long long)H * W * 3;
    const unsigned* src = reinterpret_cast<const unsigned*>(scene);
    const int nbytes = (c_hi - c_lo) * 3;
    if (nbytes > 0) {
        for (int i = threadIdx.x; i < (r_hi - r_lo) * SC_PITCH; i += 256) {
            const int r = i / SC_PITCH, d = i - r * SC_PITCH;
            const long long bs = ((sy0 + r_lo + r) * W + sx0 + c_lo) * 3;
            if (d >= ((int)(bs & 3) + nbytes + 3) / 4) continue;          // the dwords that cover the row's bytes
            const long long gd = (bs >> 2) + d;
            unsigned v;
            if (gd * 4 + 4 <= total) {
                v = src[gd];
            } else {                                       // the scene's last, partial dword: byte loads, nothing past the end
                v = 0;
                for (int k = 0; k < 4; ++k)
                    if (gd * 4 + k < total) v |= (unsigned)scene[gd * 4 + k] << (8 * k);
            }
            tile[r * SC_PITCH + d] = v;
        }
    }
    __syncthreads();
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(tile);
    const int ox = threadIdx.x & 63;
    if (ox >= cw) return;
    const size_t plane = (size_t)th * tw;
    for (int oy = threadIdx.x >> 6; oy < ch; oy += 4) {
        float* o = out + (size_t)n * 3 * plane + (size_t)(ty0 + oy) * tw + tx0 + ox;
        if (ox >= c_lo && ox < c_hi && oy >= r_lo && oy < r_hi) {
            const int shift = (int)((((sy0 + oy) * W + sx0 + c_lo) * 3) & 3);
            prep_store_pixel(bytes + (oy - r_lo) * (SC_PITCH * 4) + shift + (ox - c_lo) * 3, keep != 0, nm, o, plane);
        } else {
            o[0] = 0.f; o[plane] = 0.f; o[2 * plane] = 0.f;
        }
    }
}

LOFT_EXPORT int loft_scene_tile_prep(const uint8_t* scene, int H, int W, const int32_t* origins, int n, int th, int tw,
                                     int channels_kept, float mean0, float mean1, float mean2, float std0, float std1, float std2,
                                     float* out, void* stream) {
    if (n < 0 || H <= 0 || W <= 0 || th <= 0 || tw <= 0 || n > 65535 || loft_cdiv(th, SC_TILE) > 65535 ||
        (int64_t)H * W >= ((int64_t)1 << 31))
        return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    if (!scene || !origins || !out || ((size_t)scene & 3) || ((size_t)out & 3)) return (int)hipErrorInvalidValue;
    const PrepNorm nm = {mean0, mean1, mean2, std0, std1, std2};
    dim3 grid(loft_cdiv(tw, SC_TILE), loft_cdiv(th, SC_TILE), n);
    hipLaunchKernelGGL(scene_tile_prep_kernel, grid, dim3(256), 0, (hipStream_t)stream, scene, H, W, origins, th, tw, channels_kept,
                       nm, out);
    LOFT_LAUNCH_CHECK();
    return 0;
}

// ---- mask areas and pair intersections ------------------------------------------------------------------------------------------------
#define SP_THREADS 256
#define SP_WAVES (SP_THREADS / 64)
#define SP_MAX_S 64
#define SP_MAX_N 65536

__device__ const int32_t scene_identity_view[1] = {0};      // paste_stage_taps with V == 1: paste_sigmoid(logit), bit for bit

__device__ __forceinline__ bool scene_mask(int x, int y, const float4 b, int S, const float* taps, int H, int W, float thr) {
    return !paste_outside(x, y, b, H, W) && paste_sample(x, y, b, S, [&](int yy, int xx) -> float {
        if (yy < 0 || yy >= S || xx < 0 || xx >= S) return 0.f;
        return taps[yy * S + xx];
    }) >= thr;
}

// the number of pixels of the non-empty window w at which m(x, y) holds, to every thread: 64 pixels per wave and step, ballot and
// popcount; sh: SP_WAVES ints of LDS.  Called by the whole workgroup.
template <typename Mask>
__device__ __forceinline__ int scene_count(const PasteWin& w, Mask m, int* sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned ww = (unsigned)(w.x1 - w.x0), n = ww * (unsigned)(w.y1 - w.y0);      // n <= H * W < 2^31: p0 + 256 does not wrap
    int cnt = 0;
    for (unsigned p0 = 0; p0 < n; p0 += SP_THREADS) {                  // workgroup-uniform trip count
        const unsigned p = p0 + threadIdx.x;
        bool v = false;
        if (p < n) {
            const unsigned r = p / ww;
            v = m(w.x0 + (int)(p - r * ww), w.y0 + (int)r);
        }
        cnt += __popcll(__ballot(v));
    }
    __syncthreads();                                                   // sh free again
    if (lane == 0) sh[wave] = cnt;
    __syncthreads();
    int all = 0;
#pragma unroll
    for (int k = 0; k < SP_WAVES; ++k) all += sh[k];
    return all;
}

// recs int32 [rec_cap][3]; meta (uint64): [0] records needed, [1] nonzero when one did not fit
__global__ __launch_bounds__(SP_THREADS) void scene_pair_counts_kernel(const float* __restrict__ logits, const float* __restrict__ boxes,
                                                                       const int32_t* __restrict__ tile, int N, int S, int H, int W,
                                                                       float thr, int32_t* __restrict__ area, int32_t* recs,
                                                                       long long rec_cap, unsigned long long* meta) {
    __shared__ float taps_i[SP_MAX_S * SP_MAX_S];
    __shared__ float taps_j[SP_MAX_S * SP_MAX_S];
    __shared__ int sh_cnt[SP_WAVES];
    __shared__ int sh_hits[SP_THREADS];
    __shared__ int sh_nhit;
    const int i = blockIdx.x, tid = threadIdx.x;
    const float4 bi = reinterpret_cast<const float4*>(boxes)[i];
    const PasteWin wi = paste_window(bi, H, W);
    const int ti = tile[i];
    const bool empty = wi.x0 >= wi.x1 || wi.y0 >= wi.y1;               // workgroup-uniform
    if (empty) {
        if (tid == 0) area[i] = 0;
        return;                                                        // no pixel, no window to meet another
    }
    paste_stage_taps(taps_i, logits, i, N, 1, S, scene_identity_view);
    __syncthreads();
    const int a = scene_count(wi, [&](int x, int y) { return scene_mask(x, y, bi, S, taps_i, H, W, thr); }, sh_cnt);
    if (tid == 0) area[i] = a;

    for (int base = i + 1; base < N; base += SP_THREADS) {
        __syncthreads();                                               // the hits of the step before are consumed
        if (tid == 0) sh_nhit = 0;
        __syncthreads();
        const int jt = base + tid;                                     // one candidate per thread: the window test
        if (jt < N && tile[jt] != ti) {
            const PasteWin wj = paste_window(reinterpret_cast<const float4*>(boxes)[jt], H, W);
            if (max(wi.x0, wj.x0) < min(wi.x1, wj.x1) && max(wi.y0, wj.y0) < min(wi.y1, wj.y1)) sh_hits[atomicAdd(&sh_nhit, 1)] = jt;
        }
        __syncthreads();
        const int nhit = sh_nhit;
        for (int h = 0; h < nhit; ++h) {
            const int j = sh_hits[h];
            const float4 bj = reinterpret_cast<const float4*>(boxes)[j];
            const PasteWin wj = paste_window(bj, H, W);
            PasteWin iw;
            iw.x0 = max(wi.x0, wj.x0); iw.x1 = min(wi.x1, wj.x1); iw.y0 = max(wi.y0, wj.y0); iw.y1 = min(wi.y1, wj.y1);
            __syncthreads();                                           // taps_j free: the count of the hit before is complete
            paste_stage_taps(taps_j, logits, j, N, 1, S, scene_identity_view);
            __syncthreads();
            const int c = scene_count(iw, [&](int x, int y) {
                return scene_mask(x, y, bi, S, taps_i, H, W, thr) && scene_mask(x, y, bj, S, taps_j, H, W, thr);
            }, sh_cnt);
            if (tid == 0) {
                const unsigned long long pos = atomicAdd(&meta[0], 1ull);
                if ((long long)pos < rec_cap) {
                    recs[3 * pos] = i; recs[3 * pos + 1] = j; recs[3 * pos + 2] = c;
                } else {
                    meta[1] = 1ull;
                }
            }
        }
    }
}

LOFT_EXPORT int loft_scene_pair_counts(const float* logits, const float* boxes, const int32_t* tile, int N, int S, int H, int W,
                                       float thr, int32_t* area, int32_t* recs, int64_t rec_cap, void* meta, void* stream) {
    if (S < 1 || S > SP_MAX_S || H < 1 || W < 1 || rec_cap < 0 || N > SP_MAX_N || (int64_t)H * W >= ((int64_t)1 << 31) ||
        rec_cap > ((int64_t)1 << 31) / 3)
        return (int)hipErrorInvalidValue;
    if (!meta) return (int)hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(meta, 0, 2 * sizeof(int64_t), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    if (N <= 0) return 0;
    if (!logits || !boxes || !tile || !area || (rec_cap > 0 && !recs)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(scene_pair_counts_kernel, dim3(N), dim3(SP_THREADS), 0, (hipStream_t)stream, logits, boxes, tile, N, S, H, W, thr,
                       area, recs, (long long)rec_cap, (unsigned long long*)meta);
    LOFT_LAUNCH_CHECK();
    return 0;
}

// ---- greedy suppression over the edges ----------------------------------------------------------------------------------------------
// Edge: inter > merge_thr * min(area_i, area_j), in fp64 (both sides exact up to the one product), strict; none when an area is 0.
// Greedy in priority order (rank 0 first): a detection is suppressed iff a KEPT detection of higher priority shares an edge with it.
// One workgroup, rounds to the fixed point: per edge (hi = its endpoint of higher priority, lo = the other) with lo undecided,
// hi kept marks lo `sup`, hi undecided marks lo `wait`; then per undecided detection: sup -> suppressed, neither -> kept, else it
// waits for the next round.  The undecided detection of highest priority never waits, so every round decides one at least: at most
// N rounds.  (Not the one-shot "any better neighbour suppresses": on a chain a > b > c, b falls to a and c is then kept.)
// work int32 [3N + 2R]: state (0 undecided, 1 kept, 2 suppressed), sup, wait, the edges' hi (-1: no edge) and lo.
#define SS_THREADS 1024

__global__ __launch_bounds__(SS_THREADS) void scene_suppress_kernel(const int32_t* __restrict__ recs, long long R,
                                                                    const int32_t* __restrict__ area, const int32_t* __restrict__ rank,
                                                                    int N, double merge_thr, int32_t* work, uint8_t* __restrict__ keep) {
    __shared__ int sh_more[2];
    int32_t* state = work;
    int32_t* sup = work + N;
    int32_t* wait = work + 2 * (long long)N;
    int32_t* ehi = work + 3 * (long long)N;
    int32_t* elo = ehi + R;
    const int tid = threadIdx.x;
    if (tid < 2) sh_more[tid] = 0;
    for (int d = tid; d < N; d += SS_THREADS) { state[d] = 0; sup[d] = 0; wait[d] = 0; }
    for (long long r = tid; r < R; r += SS_THREADS) {
        const int i = recs[3 * r], j = recs[3 * r + 1], inter = recs[3 * r + 2];
        int hi = -1, lo = -1;
        if (i >= 0 && i < N && j >= 0 && j < N && i != j) {
            const int ai = area[i], aj = area[j];
            if (ai > 0 && aj > 0 && (double)inter > merge_thr * (double)min(ai, aj)) {
                const bool i_first = rank[i] < rank[j];
                hi = i_first ? i : j;
                lo = i_first ? j : i;
            }
        }
        ehi[r] = hi; elo[r] = lo;
    }
    __threadfence_block();
    __syncthreads();
    for (int round = 0; round <= N; ++round) {
        for (long long r = tid; r < R; r += SS_THREADS) {
            const int hi = ehi[r];
            if (hi < 0) continue;
            const int lo = elo[r];
            if (state[lo] != 0) continue;
            const int s = state[hi];
            if (s == 1) sup[lo] = 1;
            else if (s == 0) wait[lo] = 1;
        }
        __threadfence_block();
        __syncthreads();
        if (tid == 0) sh_more[(round + 1) & 1] = 0;                    // the next round's flag: last read before the barrier above
        bool more = false;
        for (int d = tid; d < N; d += SS_THREADS) {
            if (state[d] != 0) continue;
            if (sup[d]) state[d] = 2;
            else if (!wait[d]) state[d] = 1;
            else { wait[d] = 0; more = true; }
        }
        if (more) sh_more[round & 1] = 1;
        __threadfence_block();
        __syncthreads();
        if (!sh_more[round & 1]) break;                                // workgroup-uniform
    }
    for (int d = tid; d < N; d += SS_THREADS) keep[d] = state[d] == 1 ? 1 : 0;
}

LOFT_EXPORT int loft_scene_suppress(const int32_t* recs, int64_t R, const int32_t* area, const int32_t* rank, int N, double merge_thr,
                                    int32_t* work, uint8_t* keep, void* stream) {
    if (R < 0 || N < 0 || N > SP_MAX_N || !(merge_thr >= 0.0)) return (int)hipErrorInvalidValue;
    if (N == 0) return 0;
    if (!area || !rank || !work || !keep || (R > 0 && !recs)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(scene_suppress_kernel, dim3(1), dim3(SS_THREADS), 0, (hipStream_t)stream, recs, (long long)R, area, rank, N,
                       merge_thr, work, keep);
    LOFT_LAUNCH_CHECK();
    return 0;
}
