// resize.hip -- Resize and Pad on the device (mmdet/datasets/pipelines/transforms.py:34-349, 560-640), fused with what follows
// them in the pipeline: Resize, then one of the square's eight symmetries (RandomFlip + right-angle RandomRotate), then Normalize,
// then Pad, then HWC -> CHW, in ONE launch per batch; and the same composition for the rasterised instance bitmaps.
// Compiled with -ffp-contract=off (Normalize is image_prep.h's statement: an IEEE subtract, then an IEEE divide).
//
// The resized pixel is a per-output-pixel function of the SOURCE (no resized image exists in global memory):
//   image:  cv2.resize(INTER_LINEAR) on 8-bit pixels as include/loft_hip.h restates it -- integer taps from four small host-built
//           tables (first tap index and two int16 coefficients per output column, and per output row), or the 2 x 2 mean when the
//           source is exactly twice the target in both directions;
//   bitmap: nearest neighbour, the source index per output column / row from two host-built tables.
//
// A 64 x 64 tile of the padded canvas comes from ONE tile of at most 64 x 64 RESIZED pixels, whatever the element (d4_tile.h).  A
// workgroup builds that resized tile in LDS in the resized image's own orientation -- lanes along a resized row, so the source is
// read along rows: neighbouring lanes read neighbouring (or, when the image shrinks, regularly spaced) bytes of the same source
// rows -- and then writes the canvas tile with row-contiguous stores, picking its pixels from LDS along a row (mirrors) or along
// a column (transposes), exactly as augment.hip does.  No lane walks a column of global memory on either side.  A lane keeps its
// column's table entry in registers for all its rows; the tile's row entries sit in LDS.  Canvas pixels outside the view are 0.
#include "loft_common.h"
#include "image_prep.h"
#include "d4_tile.h"
#include "../../include/loft_hip.h"

struct ResizeGeom {
    int Hs, Ws;      // source
    int Hd, Wd;      // resized image (before the element)
    int Hp, Wp;      // padded canvas
};

// extent of the view inside canvas tile (x0, y0): clipped to [0, 64], 0 for a tile that lies in the padding altogether
__device__ __forceinline__ D4Tile resize_tile(int elem, int Hv, int Wv, int x0, int y0) {
    D4Tile t = d4_tile(elem, Hv, Wv, x0, y0);
    if (t.tw <= 0 || t.th <= 0) t.tw = t.th = t.sh = t.sw = 0;
    return t;
}

// ---- image: Resize o D4 o Normalize o Pad o HWC -> CHW ---------------------------------------------------------------------------
// img uint8 [n, Hs, Ws, 3], elems int32 [n], out fp32 [n, 3, Hp, Wp].
__global__ __launch_bounds__(256) void image_resize_prep_d4_kernel(const uint8_t* __restrict__ img, const int32_t* __restrict__ elems,
                                                                   ResizeGeom g, const int32_t* __restrict__ xofs,
                                                                   const int16_t* __restrict__ xcoef, const int32_t* __restrict__ yofs,
                                                                   const int16_t* __restrict__ ycoef, PrepNorm nm,
                                                                   float* __restrict__ out) {
    __shared__ unsigned tile[D4_TILE * D4_IMG_PITCH];
    __shared__ int row_ofs[D4_TILE];
    __shared__ int row_coef[D4_TILE];
    const int n = blockIdx.z, x0 = blockIdx.x * D4_TILE, y0 = blockIdx.y * D4_TILE;
    const int e = elems[n];
    // (a transposing entry on a non-square target loses its transpose, as in image_prep_d4_kernel: the host cannot read the table)
    const int elem = e & (g.Hd == g.Wd ? LOFT_D4_ELEMENT_MASK : LOFT_D4_ELEMENT_MASK & ~LOFT_D4_TRANSPOSE);
    const bool keep = (e & LOFT_D4_CHANNELS_KEPT) != 0;
    const D4Tile t = resize_tile(elem, g.Hd, g.Wd, x0, y0);
    const bool area = g.Ws == 2 * g.Wd && g.Hs == 2 * g.Hd;       // OpenCV's exact-half path of INTER_LINEAR
    uint8_t* bytes = reinterpret_cast<uint8_t*>(tile);
    if (threadIdx.x < t.sh) {
        const int r = t.sr0 + threadIdx.x;
        row_ofs[threadIdx.x] = area ? 2 * r : min(max(yofs[r], 0), g.Hs - 1);      // (a table is not trusted with an address)
        row_coef[threadIdx.x] = area ? 0 : *reinterpret_cast<const int*>(ycoef + 2 * r);
    }
    __syncthreads();
    const int lc = threadIdx.x & 63;
    if (lc < t.sw) {
        const int c = t.sc0 + lc;
        const int sx0 = area ? 2 * c : min(max(xofs[c], 0), g.Ws - 1);
        const int sx1 = min(sx0 + 1, g.Ws - 1);
        const int ac = area ? 0 : *reinterpret_cast<const int*>(xcoef + 2 * c);
        const int a0 = (int16_t)(ac & 0xffff), a1 = ac >> 16;
        const uint8_t* src = img + (size_t)n * g.Hs * g.Ws * 3;
        for (int r = threadIdx.x >> 6; r < t.sh; r += 4) {
            const int sy0 = row_ofs[r], sy1 = min(sy0 + 1, g.Hs - 1);
            const int bc = row_coef[r];
            const int b0 = (int16_t)(bc & 0xffff), b1 = bc >> 16;
            const uint8_t* p00 = src + ((size_t)sy0 * g.Ws + sx0) * 3;
            const uint8_t* p01 = src + ((size_t)sy0 * g.Ws + sx1) * 3;
            const uint8_t* p10 = src + ((size_t)sy1 * g.Ws + sx0) * 3;
            const uint8_t* p11 = src + ((size_t)sy1 * g.Ws + sx1) * 3;
            uint8_t* q = bytes + r * (D4_IMG_PITCH * 4) + lc * 3;
            for (int ch = 0; ch < 3; ++ch) {
                const int v00 = p00[ch], v01 = p01[ch], v10 = p10[ch], v11 = p11[ch];
                int v;
                if (area) {
                    v = (v00 + v01 + v10 + v11 + 2) >> 2;
                } else {
                    const int S0 = v00 * a0 + v01 * a1, S1 = v10 * a0 + v11 * a1;
                    v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
                }
                q[ch] = (uint8_t)v;
            }
        }
    }
    __syncthreads();
    const int ox = lc;
    if (x0 + ox >= g.Wp) return;
    const size_t plane = (size_t)g.Hp * g.Wp;
    const int th_canvas = min(D4_TILE, g.Hp - y0);
    for (int oy = threadIdx.x >> 6; oy < th_canvas; oy += 4) {
        float* o = out + (size_t)n * 3 * plane + (size_t)(y0 + oy) * g.Wp + x0 + ox;
        if (ox < t.tw && oy < t.th) {
            int r, c;
            d4_src(elem, t, ox, oy, r, c);
            prep_store_pixel(bytes + r * (D4_IMG_PITCH * 4) + c * 3, keep, nm, o, plane);
        } else {                                      // Pad(pad_val=0) comes after Normalize: exactly 0.0f
            o[0] = 0.0f;
            o[plane] = 0.0f;
            o[2 * plane] = 0.0f;
        }
    }
}

static bool resize_geom_ok(int Hs, int Ws, int Hd, int Wd, int Hp, int Wp) {
    return Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0 && Hd <= Hp && Wd <= Wp && (long)Hp * Wp < (1L << 31) &&
           loft_cdiv(Hp, D4_TILE) <= 65535;
}

LOFT_EXPORT int loft_image_resize_prep_d4(const uint8_t* img, const int32_t* elems, int n, int Hs, int Ws, int Hd, int Wd,
                                          const int32_t* xofs, const int16_t* xcoef, const int32_t* yofs, const int16_t* ycoef, int Hp,
                                          int Wp, int any_transpose, float mean0, float mean1, float mean2, float std0, float std1,
                                          float std2, float* out, void* stream) {
    if (n < 0 || n > 65535 || !resize_geom_ok(Hs, Ws, Hd, Wd, Hp, Wp) || (any_transpose && Hd != Wd)) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    if (!img || !elems || !xofs || !xcoef || !yofs || !ycoef || !out || ((size_t)xcoef & 3) || ((size_t)ycoef & 3) || ((size_t)out & 3))
        return (int)hipErrorInvalidValue;
    const ResizeGeom g = {Hs, Ws, Hd, Wd, Hp, Wp};
    const PrepNorm nm = {mean0, mean1, mean2, std0, std1, std2};
    dim3 grid(loft_cdiv(Wp, D4_TILE), loft_cdiv(Hp, D4_TILE), n);
    hipLaunchKernelGGL(image_resize_prep_d4_kernel, grid, dim3(256), 0, (hipStream_t)stream, img, elems, g, xofs, xcoef, yofs, ycoef, nm,
                       out);
    LOFT_LAUNCH_CHECK();
    return 0;
}

// ---- instance bitmaps: nearest-neighbour Resize o D4 o Pad -----------------------------------------------------------------------
// in uint8 [K, Hs, Ws], out uint8 [K, Hp, Wp], ONE element for the K bitmaps of a sample.  The resized tile sits in LDS in
// mask_d4_kernel's layout and the canvas tile is written by the same lanes: one lane per output dword, rows as there.
__global__ __launch_bounds__(256) void mask_resize_d4_kernel(const uint8_t* __restrict__ in, int elem, ResizeGeom g,
                                                             const int32_t* __restrict__ xidx, const int32_t* __restrict__ yidx,
                                                             uint8_t* __restrict__ out) {
    __shared__ unsigned tile[D4_TILE * D4_MASK_PITCH + 2];
    __shared__ int row_idx[D4_TILE];
    const int k = blockIdx.z, x0 = blockIdx.x * D4_TILE, y0 = blockIdx.y * D4_TILE;
    const D4Tile t = resize_tile(elem, g.Hd, g.Wd, x0, y0);
    uint8_t* bytes = reinterpret_cast<uint8_t*>(tile);
    if (threadIdx.x < t.sh) row_idx[threadIdx.x] = min(max(yidx[t.sr0 + threadIdx.x], 0), g.Hs - 1);
    __syncthreads();
    const int lc = threadIdx.x & 63;
    if (lc < t.sw) {
        const uint8_t* src = in + (size_t)k * g.Hs * g.Ws + min(max(xidx[t.sc0 + lc], 0), g.Ws - 1);
        for (int r = threadIdx.x >> 6; r < t.sh; r += 4) bytes[mask_lds_row(r) * 4 + lc] = src[(size_t)row_idx[r] * g.Ws];
    }
    __syncthreads();
    const int gq = threadIdx.x & 15, q = threadIdx.x >> 4;
    if (x0 + 4 * gq >= g.Wp) return;                  // Wp % 4 == 0: whole dwords
    const int row16 = (elem & LOFT_D4_TRANSPOSE) ? (q >> 1) + 8 * (q & 1) : q;
    unsigned* dst = reinterpret_cast<unsigned*>(out + (size_t)k * g.Hp * g.Wp);
    const int th_canvas = min(D4_TILE, g.Hp - y0);
    for (int oy = row16; oy < th_canvas; oy += 16) {
        unsigned v = 0;
        for (int j = 0; j < 4; ++j) {
            const int ox = 4 * gq + j;
            if (ox < t.tw && oy < t.th) {
                int r, c;
                d4_src(elem, t, ox, oy, r, c);
                v |= (unsigned)bytes[mask_lds_row(r) * 4 + c] << (8 * j);
            }
        }
        dst[((size_t)(y0 + oy) * g.Wp + x0) / 4 + gq] = v;
    }
}

LOFT_EXPORT int loft_mask_resize_d4_u8(const uint8_t* masks, int K, int Hs, int Ws, int Hd, int Wd, const int32_t* xidx,
                                       const int32_t* yidx, int Hp, int Wp, int elem, uint8_t* out, void* stream) {
    if (K < 0 || K > 65535 || !resize_geom_ok(Hs, Ws, Hd, Wd, Hp, Wp) || (Wp & 3) || (elem & ~LOFT_D4_ELEMENT_MASK) ||
        ((elem & LOFT_D4_TRANSPOSE) && Hd != Wd))
        return (int)hipErrorInvalidValue;
    if (K == 0) return 0;
    if (!masks || !xidx || !yidx || !out || masks == out || ((size_t)out & 3)) return (int)hipErrorInvalidValue;
    const ResizeGeom g = {Hs, Ws, Hd, Wd, Hp, Wp};
    dim3 grid(loft_cdiv(Wp, D4_TILE), loft_cdiv(Hp, D4_TILE), K);
    hipLaunchKernelGGL(mask_resize_d4_kernel, grid, dim3(256), 0, (hipStream_t)stream, masks, elem, g, xidx, yidx, out);
    LOFT_LAUNCH_CHECK();
    return 0;
}
