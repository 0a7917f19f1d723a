// mask_rle.hip -- the mask head's class-selected logits straight to the bytes of pycocotools' compressed RLE strings: what
// bonai_amd/rle.py rle_encode_masks makes of the bitmaps of loft_mask_paste / loft_mask_paste_views / loft_mask_translate
// (mmdet/apis/test.py:59-67 encode_mask_results -> mask_util.encode; cocoapi maskApi.c rleEncode + rleToString), without the
// [N, img_h, img_w] bitmaps: a pasted mask is zero outside its box's tight window, so only the window's pixels are evaluated.
//
// The mask is the paste kernels' (box_codec.h): taps = the merged probabilities of mask_paste_views_kernel (paste_stage_taps; V == 1
// with the identity element: mask_paste_kernel's sigmoid), pixel (x, y) set iff !paste_outside && paste_sample >= thr.  With offsets
// the result is the FOOTPRINT, mask_translate_kernel's shift of that roof: footprint(y, x) = roof(y + lroundf(dy), x + lroundf(dx)),
// zero where the source lies outside the image; its window is the roof's moved by -(ox, oy) and clipped.
// Runs are column-major (p = x * img_h + y): a run starts at p iff m[p] != m[p - 1], m[-1] = 0; counts = differences of the start
// positions, the first one the leading run of zeros (0 when m[0] = 1).  A run that reaches the bottom of a column continues into the
// top of the next one.
//
// One workgroup of four waves per detection, three sweeps:
//   1. a wave takes a window column at a time, 64 pixels per step: ballot of the mask, run starts = ballot ^ (ballot << 1 | carry),
//      popcount into the column's LDS counter; block scan of the counters -> R run starts, and a segment of R positions reserved in
//      the `runs` scratch with one atomic add on a cursor
//   2. the same walk again, every start position stored at its rank in the segment
//   3. one thread per count: count i = q[i] - q[i-1] (q = the positions, q[-1] = 0, q[R] = img_h * img_w), from the fourth on minus
//      the count two places back; its character length; block scan -> byte positions in a segment reserved on a second cursor; the
//      characters (5 data bits each, 0x20 = more follow, sign carried by bit 0x10, + 48) written with byte stores
// The bytes of a detection depend on nothing but its inputs; only where its two segments lie depends on the order the workgroups
// reach the cursors.  meta (int64): [0] positions needed, [1] bytes needed, [2] nonzero when a segment did not fit (nothing is
// written past a capacity; a detection whose positions did not fit adds an upper bound of its bytes to [1], so capacities of
// ([0], [1]) always suffice for a second launch), [4 + 2n], [5 + 2n] = (byte offset, byte length) of detection n, offset -1 when it
// did not fit.  Device memory: the two segments' buffers, proportional to the number of runs.  Built with -ffp-contract=off.
#include "loft_common.h"
#include "box_codec.h"
#include "../../include/loft_hip.h"

#define RLE_THREADS 256
#define RLE_WAVES (RLE_THREADS / 64)
#define RLE_MAX_S 64
#define RLE_MAX_VIEWS 8
#define RLE_MAX_W 8192      // window columns with an LDS counter each

struct RleWin { int x0, x1, y0, y1, ox, oy; };      // the (footprint's) window [x0, x1) x [y0, y1) and the shift to the roof

// exclusive prefix of v over the workgroup's threads, total to all; sh: RLE_WAVES ints of LDS
__device__ __forceinline__ int rle_block_scan(int v, int* sh, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    __syncthreads();                                   // sh free again
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < RLE_WAVES; ++w) {
        const int s = sh[w];
        if (w < wave) before += s;
        all += s;
    }
    total = all;
    return before + inc - v;
}

// one wave walks column j of the window; returns its number of run starts (wave-uniform) and, WRITE, stores their positions at
// dst[0..) in ascending order
template <bool WRITE, typename Mask>
__device__ __forceinline__ int rle_column(int j, const RleWin& w, int img_h, Mask M, int32_t* dst) {
    const int lane = threadIdx.x & 63;
    const int x = w.x0 + j;
    const bool body = x < w.x1;                        // else: the column after the window, for the run that ends at its top
    // the pixel before the column's top is (x - 1, img_h - 1): in the window only when the window reaches the bottom
    const bool pb = (w.y1 == img_h && j > 0) ? M(x - 1, img_h - 1) : false;
    int cnt = 0;
    unsigned long long carry = 0;
    if (w.y0 > 0 || !body) {                           // (x, 0) is outside the window: a run from the column before ends here
        if (pb) {
            if (WRITE && lane == 0) dst[0] = x * img_h;
            cnt = 1;
        }
    } else {
        carry = pb ? 1ull : 0ull;
    }
    if (body) {
        const int ye = min(w.y1 + 1, img_h);           // the pixel below the window closes an open run
        for (int yb = w.y0; yb < ye; yb += 64) {
            const int y = yb + lane;
            const bool m = y < w.y1 && M(x, y);
            const unsigned long long bits = __ballot(m);
            unsigned long long chg = bits ^ ((bits << 1) | carry);
            if (ye - yb < 64) chg &= (1ull << (ye - yb)) - 1ull;
            if (WRITE && ((chg >> lane) & 1ull)) dst[cnt + __popcll(chg & ((1ull << lane) - 1ull))] = x * img_h + y;
            cnt += __popcll(chg);
            carry = bits >> 63;
        }
    }
    return cnt;
}

// count i of a mask with start positions q[0..R): rleToString's value (the count, from the fourth on minus the count two back)
__device__ __forceinline__ int rle_q(const int32_t* q, int i, int R, int hw) { return i < 0 ? 0 : (i < R ? q[i] : hw); }
__device__ __forceinline__ int rle_value(const int32_t* q, int i, int R, int hw) {
    int c = rle_q(q, i, R, hw) - rle_q(q, i - 1, R, hw);
    if (i > 2) c -= rle_q(q, i - 2, R, hw) - rle_q(q, i - 3, R, hw);
    return c;
}
template <bool WRITE>
__device__ __forceinline__ int rle_chars(int x, uint8_t* dst) {
    int len = 0;
    bool more;
    do {
        int ch = x & 0x1f;
        x >>= 5;                                       // arithmetic
        more = (ch & 0x10) ? x != -1 : x != 0;
        if (more) ch |= 0x20;
        if (WRITE) dst[len] = (uint8_t)(ch + 48);
        ++len;
    } while (more);
    return len;
}

__global__ __launch_bounds__(RLE_THREADS) void mask_rle_kernel(const float* __restrict__ logits, const float* __restrict__ boxes,
                                                               const float* __restrict__ offsets, int N, int V, int S,
                                                               const int32_t* __restrict__ views, int img_h, int img_w, float thr,
                                                               int32_t* runs, long long run_cap, uint8_t* out, long long byte_cap,
                                                               int max_chars, unsigned long long* meta) {
    __shared__ float taps[RLE_MAX_S * RLE_MAX_S];
    __shared__ int sh_scan[RLE_WAVES];
    __shared__ long long sh_base;
    extern __shared__ int colcnt[];                    // img_w counters
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hw = img_h * img_w;
    const float4 b = reinterpret_cast<const float4*>(boxes)[n];
    paste_stage_taps(taps, logits, n, N, V, S, views);
    __syncthreads();
    auto at = [&](int yy, int xx) -> float {
        if (yy < 0 || yy >= S || xx < 0 || xx >= S) return 0.f;
        return taps[yy * S + xx];
    };
    // the roof's window: the pixels paste_outside does not exclude (its bounds are whole numbers), then moved by the offset
    RleWin w;
    w.ox = 0; w.oy = 0;
    if (offsets) {
        const long lx = lroundf(offsets[2 * n]), ly = lroundf(offsets[2 * n + 1]);
        // a shift of a whole image or more leaves nothing, like any larger one
        w.ox = (int)(lx < -img_w ? -img_w : (lx > img_w ? img_w : lx));
        w.oy = (int)(ly < -img_h ? -img_h : (ly > img_h ? img_h : ly));
    }
    const PasteWin roof = paste_window(b, img_h, img_w);
    w.x0 = max(roof.x0 - w.ox, 0);
    w.x1 = min(roof.x1 - w.ox, img_w);
    w.y0 = max(roof.y0 - w.oy, 0);
    w.y1 = min(roof.y1 - w.oy, img_h);
    auto M = [&](int x, int y) -> bool {
        const int sx = x + w.ox, sy = y + w.oy;
        if (sx < 0 || sx >= img_w || sy < 0 || sy >= img_h) return false;
        return !paste_outside(sx, sy, b, img_h, img_w) && paste_sample(sx, sy, b, S, at) >= thr;
    };
    int ncol = 0;
    if (w.x0 < w.x1 && w.y0 < w.y1) ncol = (w.x1 - w.x0) + ((w.y1 == img_h && w.x1 < img_w) ? 1 : 0);

    // ---- sweep 1: run starts per column, their exclusive prefix
    for (int j = wave; j < ncol; j += RLE_WAVES) {
        const int c = rle_column<false>(j, w, img_h, M, nullptr);
        if (lane == 0) colcnt[j] = c;
    }
    __syncthreads();
    const int per = (ncol + RLE_THREADS - 1) / RLE_THREADS;
    const int lo = min(tid * per, ncol), hi = min(lo + per, ncol);
    int mine = 0;
    for (int j = lo; j < hi; ++j) mine += colcnt[j];
    int R;
    int run = rle_block_scan(mine, sh_scan, R);
    for (int j = lo; j < hi; ++j) {
        const int c = colcnt[j];
        colcnt[j] = run;
        run += c;
    }
    if (tid == 0) sh_base = R ? (long long)atomicAdd(&meta[0], (unsigned long long)R) : 0ll;
    __syncthreads();
    const long long rbase = sh_base;
    if (R && rbase + R > run_cap) {
        if (tid == 0) {
            atomicAdd(&meta[1], (unsigned long long)max_chars * (unsigned long long)(R + 1));
            meta[2] = 1ull;
            meta[4 + 2 * n] = (unsigned long long)-1ll;
            meta[5 + 2 * n] = 0ull;
        }
        return;
    }
    int32_t* q = runs + rbase;

    // ---- sweep 2: the start positions, in order
    for (int j = wave; j < ncol; j += RLE_WAVES) rle_column<true>(j, w, img_h, M, q + colcnt[j]);
    __threadfence_block();
    __syncthreads();

    // ---- sweep 3: R + 1 counts -> characters
    int len_sum = 0;
    for (int i = tid; i <= R; i += RLE_THREADS) len_sum += rle_chars<false>(rle_value(q, i, R, hw), nullptr);
    int L;
    rle_block_scan(len_sum, sh_scan, L);
    __syncthreads();                                   // sh_base read by all before it is written again
    if (tid == 0) sh_base = (long long)atomicAdd(&meta[1], (unsigned long long)L);
    __syncthreads();
    const long long bbase = sh_base;
    if (bbase + L > byte_cap) {
        if (tid == 0) {
            meta[2] = 1ull;
            meta[4 + 2 * n] = (unsigned long long)-1ll;
            meta[5 + 2 * n] = (unsigned long long)L;
        }
        return;
    }
    if (tid == 0) {
        meta[4 + 2 * n] = (unsigned long long)bbase;
        meta[5 + 2 * n] = (unsigned long long)L;
    }
    uint8_t* dst = out + bbase;
    int done = 0;
    for (int i0 = 0; i0 <= R; i0 += RLE_THREADS) {     // workgroup-uniform trip count
        const int i = i0 + tid;
        const int v = i <= R ? rle_value(q, i, R, hw) : 0;
        const int len = i <= R ? rle_chars<false>(v, nullptr) : 0;
        int tot;
        const int at_byte = rle_block_scan(len, sh_scan, tot);
        if (i <= R) rle_chars<true>(v, dst + done + at_byte);
        done += tot;
    }
}

LOFT_EXPORT int loft_mask_rle(const float* logits, const float* boxes, const float* offsets, int N, int V, int S, const int32_t* views,
                              int img_h, int img_w, float thr, void* runs, int64_t run_cap, uint8_t* out, int64_t byte_cap, void* meta,
                              void* stream) {
    if (V < 1 || V > RLE_MAX_VIEWS || S < 1 || S > RLE_MAX_S || img_h < 1 || img_w < 1 || img_w > RLE_MAX_W || run_cap < 0 ||
        byte_cap < 0)
        return (int)hipErrorInvalidValue;
    if ((int64_t)img_h * img_w >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
    if (N <= 0) return 0;
    if (N > 65535) return (int)hipErrorInvalidValue;
    // the longest string of one count: |value| <= img_h * img_w needs k characters with 2^(5k - 1) > img_h * img_w
    int max_chars = 1;
    while (((int64_t)1 << (5 * max_chars - 1)) <= (int64_t)img_h * img_w) ++max_chars;
    hipError_t e = hipMemsetAsync(meta, 0, 4 * sizeof(int64_t), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(mask_rle_kernel, dim3(N), dim3(RLE_THREADS), (size_t)img_w * sizeof(int), (hipStream_t)stream, logits, boxes,
                       offsets, N, V, S, views, img_h, img_w, thr, (int32_t*)runs, (long long)run_cap, out, (long long)byte_cap,
                       max_chars, (unsigned long long*)meta);
    LOFT_LAUNCH_CHECK();
    return 0;
}
