// stem_wgrad.hip -- backward of the trainable ResNet stem (frozen_stages < 0) in one launch:
//   p = maxpool3x3/2(y),  y = relu(conv7x7/2(img) * bn_scale + bn_shift)        (mmdet/models/backbones/resnet.py:628-631)
// The image needs no gradient, so the backward is the gradient of the BN-folded weight and of the BN shift:
//   dpre[b,oy,ox,n] = (y > 0) * sum over the <= 4 pool windows containing (oy,ox) of gp[window] * [(oy,ox) is its argmax]
//   dwp[t=(r,s)][n][c] += sum dpre[b,oy,ox,n] * img[b,c,2oy-3+r,2ox-3+s],   db[n] += sum dpre[b,oy,ox,n]
// in the [tap][Cout][Cin] + [Cout] fp32 form loft_fold_unpack_bwd consumes.  dpre never exists in HBM.
//
// Tile = 4 x 8 pool windows.  Their 3x3 footprints cover 9 x 17 pixels of y (the tile's own windows need no halo beyond that),
// and those need a 23 x 39 window of the image.  The pixels on the tile's rim also belong to windows of the neighbouring tiles:
// each tile contracts only the share of dpre that ITS windows send (the contraction is linear in dpre, the shares add up in
// the accumulators), so y is fetched 153/128 times and nothing else is shared between tiles.
// Per tile:  A  argmax of each window x channel, recomputed from the y tile with F.max_pool2d's rule (first maximum in
//               (ky, kx) scan order, padding never wins): no index map is stored by the forward;
//            B  dpre of the 153 pixels x 64 channels in LDS (gather over the <= 4 windows of the tile, ReLU mask);
//            C  contraction over the pixels: 16-bit form on the matrix cores (M = 64 channels, N = 147 (c, r, s) columns + a
//               column of ones that yields db, padded to 192; the im2col fragments are gathered from the fp32 image window in
//               LDS); fp32 form (parity mode) as plain fp32 FMA chains.
// Accumulators stay in registers over the tiles of a persistent workgroup and leave once, staged through LDS so that every
// wave's atomic add covers 256 contiguous bytes of dwp.
#include "loft_common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

__device__ __forceinline__ void ld8(const bf16_t* p, float v[8]) { unpack8_16(*reinterpret_cast<const uint4*>(p), v); }
__device__ __forceinline__ void ld8(const float* p, float v[8]) { ld4(p, v); ld4(p + 4, v + 4); }
__device__ __forceinline__ void st8(float* p, const float v[8]) { st4(p, v); st4(p + 4, v + 4); }
// raw 8-element copy (no conversion)
__device__ __forceinline__ void cp8(bf16_t* d, const bf16_t* s) { *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(s); }
__device__ __forceinline__ void cp8(float* d, const float* s) {
    reinterpret_cast<float4*>(d)[0] = reinterpret_cast<const float4*>(s)[0];
    reinterpret_cast<float4*>(d)[1] = reinterpret_cast<const float4*>(s)[1];
}
__device__ __forceinline__ void zero8(bf16_t* d) { *reinterpret_cast<uint4*>(d) = make_uint4(0, 0, 0, 0); }
__device__ __forceinline__ void zero8(float* d) {
    reinterpret_cast<float4*>(d)[0] = make_float4(0.f, 0.f, 0.f, 0.f);
    reinterpret_cast<float4*>(d)[1] = make_float4(0.f, 0.f, 0.f, 0.f);
}

constexpr int SW_WY = 4, SW_WX = 8, SW_NWIN = SW_WY * SW_WX;                 // pool windows of a tile
constexpr int SW_YR = 2 * SW_WY + 1, SW_YC = 2 * SW_WX + 1;                  // their footprint in y: 9 x 17 pixels
constexpr int SW_NPIX = SW_YR * SW_YC, SW_NPIXP = 160;                       // 153, padded to 10 MFMA steps of 16
constexpr int SW_PR = 2 * (SW_YR - 1) + 7, SW_PC = 2 * (SW_YC - 1) + 7, SW_PP = 40;   // image window 23 x 39, row pitch 40
constexpr int SW_K = 147, SW_DTP = SW_NPIXP + 8;                             // im2col columns; pitch of the transposed dpre
constexpr int SW_STAGE_P = 65;                                               // flush stage [148][64], pitch 65

template <typename T>
struct SwLds {
    static constexpr int ytile = 0;                                          // [153][64] T   (fp32 form: dpre in place)
    static constexpr int gpt = ytile + SW_NPIX * 64 * (int)sizeof(T);        // [32][64] T
    static constexpr int amax = gpt + SW_NWIN * 64 * (int)sizeof(T);         // [32][64] bytes
    static constexpr int patch = amax + SW_NWIN * 64;                        // [3][23][40] fp32
    static constexpr int pixoff = patch + 3 * SW_PR * SW_PP * 4;             // [160] int
    static constexpr int dT = pixoff + SW_NPIXP * 4;                         // 16-bit form: [64][168] 16-bit
    static constexpr int total = dT + (sizeof(T) == 2 ? 64 * SW_DTP * 2 : 0);
    static_assert(total <= 65536 && (SW_K + 1) * SW_STAGE_P * 4 <= total, "LDS budget");
    static_assert(gpt % 16 == 0 && amax % 16 == 0 && patch % 16 == 0 && pixoff % 16 == 0 && dT % 16 == 0, "LDS alignment");
};

template <typename T>
__global__ __launch_bounds__(256) void stem7x7_pool_wgrad_kernel(const float* __restrict__ img, const T* __restrict__ y,
                                                                 const T* __restrict__ gp, float* __restrict__ dwp,
                                                                 float* __restrict__ db, int B, int H, int W, int Hy, int Wy,
                                                                 int Hp, int Wp, int tiles_x, int tiles_y) {
    constexpr bool MF = sizeof(T) == 2;
    typedef SwLds<T> Lo;
    __shared__ __attribute__((aligned(16))) char lds[Lo::total];
    T* ytile = reinterpret_cast<T*>(lds + Lo::ytile);
    T* gpt = reinterpret_cast<T*>(lds + Lo::gpt);
    unsigned char* amax = reinterpret_cast<unsigned char*>(lds + Lo::amax);
    float* patch = reinterpret_cast<float*>(lds + Lo::patch);
    int* pixoff = reinterpret_cast<int*>(lds + Lo::pixoff);
    bf16_t* dT = reinterpret_cast<bf16_t*>(lds + Lo::dT);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int frow = lane & 31, fq = lane >> 5;

    // offset of pixel p's 7x7 window in the image patch (pad pixels 153..159 point at pixel 152: finite values x dpre = 0)
    for (int i = tid; i < SW_NPIXP; i += 256) {
        const int p = i < SW_NPIX ? i : SW_NPIX - 1;
        pixoff[i] = 2 * (p / SW_YC) * SW_PP + 2 * (p % SW_YC);
    }
    if constexpr (MF)
        for (int i = tid; i < 64 * (SW_DTP - SW_NPIX); i += 256)
            dT[(i / (SW_DTP - SW_NPIX)) * SW_DTP + SW_NPIX + i % (SW_DTP - SW_NPIX)] = 0;

    // ---- accumulators.  16-bit form: wave -> 32 channels (mt) x 3 column blocks of 32 (ntb..ntb+2), lane's column k = nt*32 + frow
    //      fp32 form: thread (n = tid & 63, kq = tid >> 6) -> channel n x columns k = kq + 4q
    const int mt = wave & 1, ntb = (wave >> 1) * 3;
    f32x16 acc[3];
    int koff[3], kind[3];                      // kind: 0 = image column, 1 = the column of ones (db), 2 = zero padding
    float facc[37], faccb = 0.f;
    int fkoff[37];
    if constexpr (MF) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
            const int k = (ntb + j) * 32 + frow;
            kind[j] = k < SW_K ? 0 : (k == SW_K ? 1 : 2);
            const int kk = k < SW_K ? k : 0;
            const int c = kk / 49, rs = kk - c * 49, r = rs / 7, s = rs - r * 7;
            koff[j] = (c * SW_PR + r) * SW_PP + s;
        }
    } else {
#pragma unroll
        for (int q = 0; q < 37; ++q) {
            facc[q] = 0.f;
            const int k = (tid >> 6) + 4 * q;
            const int kk = k < SW_K ? k : 0;
            const int c = kk / 49, rs = kk - c * 49, r = rs / 7, s = rs - r * 7;
            fkoff[q] = (c * SW_PR + r) * SW_PP + s;
        }
    }

    const int ntiles = tiles_x * tiles_y * B;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int tt = t;
        const int tx0 = tt % tiles_x; tt /= tiles_x;
        const int ty0 = tt % tiles_y;
        const int b = tt / tiles_y;
        const int py0 = ty0 * SW_WY, px0 = tx0 * SW_WX;          // first pool window
        const int yr0 = 2 * py0 - 1, xc0 = 2 * px0 - 1;          // first y pixel of the footprint
        const int iy0 = 2 * yr0 - 3, ix0 = 2 * xc0 - 3;          // first image pixel of the patch
        __syncthreads();                                         // the previous tile's contraction has read everything
        {
            const float* ib = img + (long)b * 3 * H * W;
            for (int i = tid; i < 3 * SW_PR * SW_PP; i += 256) {
                const int col = i % SW_PP, rr = i / SW_PP, r = rr % SW_PR, c = rr / SW_PR;
                const int iy = iy0 + r, ix = ix0 + col;
                float x = 0.f;
                if (col < SW_PC && iy >= 0 && iy < H && ix >= 0 && ix < W) x = ib[((long)c * H + iy) * W + ix];
                patch[i] = x;
            }
        }
        for (int i = tid; i < SW_NPIX * 8; i += 256) {
            const int pix = i >> 3, c8 = i & 7;
            const int ay = yr0 + pix / SW_YC, ax = xc0 + pix % SW_YC;
            T* d = ytile + pix * 64 + c8 * 8;
            if (ay >= 0 && ay < Hy && ax >= 0 && ax < Wy) cp8(d, y + (((long)b * Hy + ay) * Wy + ax) * 64 + c8 * 8);
            else zero8(d);
        }
        const int win = tid >> 3, wc8 = tid & 7, wy = win >> 3, wx = win & 7;     // 32 windows x 8 channel groups = 256 threads
        const bool wvalid = py0 + wy < Hp && px0 + wx < Wp;
        {
            T* d = gpt + win * 64 + wc8 * 8;
            if (wvalid) cp8(d, gp + (((long)b * Hp + py0 + wy) * Wp + px0 + wx) * 64 + wc8 * 8);
            else zero8(d);
        }
        __syncthreads();
        // ---- A: argmax of window (wy, wx), channels wc8*8 .. +8: strict '>' in (ky, kx) order keeps the FIRST maximum
        {
            float best[8];
            unsigned idx[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) { best[q] = -__builtin_inff(); idx[q] = 15u; }
            if (wvalid) {
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    const int ay = yr0 + 2 * wy + ky;
                    if (ay < 0 || ay >= Hy) continue;
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const int ax = xc0 + 2 * wx + kx;
                        if (ax < 0 || ax >= Wy) continue;
                        float v[8];
                        ld8(ytile + ((2 * wy + ky) * SW_YC + 2 * wx + kx) * 64 + wc8 * 8, v);
#pragma unroll
                        for (int q = 0; q < 8; ++q)
                            if (v[q] > best[q]) { best[q] = v[q]; idx[q] = (unsigned)(ky * 3 + kx); }
                    }
                }
            }
            uint2 pk;
            pk.x = idx[0] | (idx[1] << 8) | (idx[2] << 16) | (idx[3] << 24);
            pk.y = idx[4] | (idx[5] << 8) | (idx[6] << 16) | (idx[7] << 24);
            *reinterpret_cast<uint2*>(amax + win * 64 + wc8 * 8) = pk;
        }
        __syncthreads();
        // ---- B: dpre of footprint pixel (yy, xx): window (wy2, wx2) of the tile covers rows 2wy2 .. 2wy2+2, cols 2wx2 .. 2wx2+2
        for (int i = tid; i < SW_NPIX * 8; i += 256) {
            const int pix = i >> 3, c8 = i & 7;
            const int yy = pix / SW_YC, xx = pix % SW_YC;
            float yv[8], d[8];
            ld8(ytile + pix * 64 + c8 * 8, yv);
#pragma unroll
            for (int q = 0; q < 8; ++q) d[q] = 0.f;
            const int wy_lo = yy >= 2 ? (yy - 1) >> 1 : 0, wy_hi = (yy >> 1) < SW_WY ? (yy >> 1) : SW_WY - 1;
            const int wx_lo = xx >= 2 ? (xx - 1) >> 1 : 0, wx_hi = (xx >> 1) < SW_WX ? (xx >> 1) : SW_WX - 1;
            for (int wy2 = wy_lo; wy2 <= wy_hi; ++wy2)
                for (int wx2 = wx_lo; wx2 <= wx_hi; ++wx2) {
                    const unsigned pos = (unsigned)((yy - 2 * wy2) * 3 + (xx - 2 * wx2));
                    const int w2 = wy2 * SW_WX + wx2;
                    const uint2 am = *reinterpret_cast<const uint2*>(amax + w2 * 64 + c8 * 8);
                    float g[8];
                    ld8(gpt + w2 * 64 + c8 * 8, g);
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const unsigned a = ((q < 4 ? am.x : am.y) >> (8 * (q & 3))) & 0xffu;
                        if (a == pos) d[q] += g[q];
                    }
                }
#pragma unroll
            for (int q = 0; q < 8; ++q) d[q] = yv[q] > 0.f ? d[q] : 0.f;
            if constexpr (MF) {
#pragma unroll
                for (int q = 0; q < 8; ++q) dT[(c8 * 8 + q) * SW_DTP + pix] = f32_to_bf16(d[q]);
            } else {
                st8(reinterpret_cast<float*>(ytile) + pix * 64 + c8 * 8, d);
            }
        }
        __syncthreads();
        // ---- C: contraction over the tile's pixels
        if constexpr (MF) {
#pragma unroll 2
            for (int ks = 0; ks < SW_NPIXP / 16; ++ks) {
                const int p0 = ks * 16 + fq * 8;
                const bf16x8 a = *reinterpret_cast<const bf16x8*>(dT + (mt * 32 + frow) * SW_DTP + p0);
                const int4 po0 = *reinterpret_cast<const int4*>(pixoff + p0);
                const int4 po1 = *reinterpret_cast<const int4*>(pixoff + p0 + 4);
                const int po[8] = {po0.x, po0.y, po0.z, po0.w, po1.x, po1.y, po1.z, po1.w};
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    if ((ntb + j) * 32 > SW_K) continue;           // a block of padding columns only (wave-uniform)
                    float xv[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float v = patch[po[e] + koff[j]];
                        xv[e] = kind[j] == 0 ? v : (kind[j] == 1 ? 1.f : 0.f);
                    }
                    const uint4 bw = pack8_16(xv);
                    acc[j] = LOFT_MFMA_32x32x16(a, __builtin_bit_cast(bf16x8, bw), acc[j]);
                }
            }
        } else {
            const float* dpre = reinterpret_cast<const float*>(ytile);
            const int n = tid & 63;
            for (int p = 0; p < SW_NPIX; ++p) {
                const float d = dpre[p * 64 + n];
                const float* pm = patch + pixoff[p];
                faccb += d;
#pragma unroll
                for (int q = 0; q < 37; ++q) facc[q] = fmaf(d, pm[fkoff[q]], facc[q]);
            }
        }
    }

    // ---- flush: stage[k][n] (k = c*49 + tap; k = 147: db) in LDS, then atomics in the linear order of dwp [tap][n][c]
    __syncthreads();
    float* stage = reinterpret_cast<float*>(lds);
    if constexpr (MF) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int k = (ntb + j) * 32 + frow;
            if (k <= SW_K) {
#pragma unroll
                for (int r = 0; r < 16; ++r) stage[k * SW_STAGE_P + mt * 32 + 8 * (r >> 2) + 4 * fq + (r & 3)] = acc[j][r];
            }
        }
    } else {
        const int n = tid & 63, kq = tid >> 6;
#pragma unroll
        for (int q = 0; q < 37; ++q) {
            const int k = kq + 4 * q;
            if (k < SW_K) stage[k * SW_STAGE_P + n] = facc[q];
        }
        if (kq == 0) stage[SW_K * SW_STAGE_P + n] = faccb;
    }
    __syncthreads();
    for (int o = tid; o < 49 * 64 * 3; o += 256) {
        const int c = o % 3, tn = o / 3, n = tn & 63, tap = tn >> 6;
        unsafeAtomicAdd(dwp + o, stage[(c * 49 + tap) * SW_STAGE_P + n]);
    }
    if (tid < 64) unsafeAtomicAdd(db + tid, stage[SW_K * SW_STAGE_P + tid]);
}

}  // namespace

LOFT_EXPORT int loft_stem7x7_pool_wgrad(const float* img, const void* y, const void* gp, float* dwp, float* db, int dtype, int B,
                                        int H, int W, void* stream) {
    if (dtype != LOFT_F32 && dtype != LOFT_ACT16) return (int)hipErrorInvalidValue;   // the other build's 16-bit type
    if (!img || !y || !gp || !dwp || !db || B < 1 || H < 1 || W < 1) return (int)hipErrorInvalidValue;
    const int Hy = (H + 6 - 7) / 2 + 1, Wy = (W + 6 - 7) / 2 + 1;            // conv 7x7 / 2 / pad 3
    const int Hp = (Hy + 2 - 3) / 2 + 1, Wp = (Wy + 2 - 3) / 2 + 1;          // max pool 3x3 / 2 / pad 1
    const int tiles_x = loft_cdiv(Wp, SW_WX), tiles_y = loft_cdiv(Hp, SW_WY);
    const long ntiles = (long)tiles_x * tiles_y * B;
    if (ntiles > 0x7fffffffL) return (int)hipErrorInvalidValue;
    const int blocks = ntiles < 512 ? (int)ntiles : 512;                     // two persistent workgroups per CU
    if (dtype == LOFT_F32)
        hipLaunchKernelGGL(stem7x7_pool_wgrad_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, img, (const float*)y,
                           (const float*)gp, dwp, db, B, H, W, Hy, Wy, Hp, Wp, tiles_x, tiles_y);
    else
        hipLaunchKernelGGL(stem7x7_pool_wgrad_kernel<bf16_t>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, img,
                           (const bf16_t*)y, (const bf16_t*)gp, dwp, db, B, H, W, Hy, Wy, Hp, Wp, tiles_x, tiles_y);
    LOFT_LAUNCH_CHECK();
    return 0;
}
