// augment.hip -- image-level augmentation on the device: the eight symmetries of the square (RandomFlip + right-angle
// RandomRotate, mmdet/datasets/pipelines/transforms.py:406-456, 1837-2096) applied to the uploaded uint8 tiles and to the
// rasterised instance bitmaps.  HBM bound: every byte is read once and written once.
// Compiled with -ffp-contract=off: Normalize is an IEEE subtract followed by an IEEE divide, bit for bit what the torch chain
// of data.to_device_batch (x.float(), channel reversal, (x - mean) / std, permute) produces.
//
// An element (include/loft_hip.h LOFT_D4_*) is an optional transpose, then an optional x-mirror, then an optional y-mirror:
//     out[y][x] = in[r][c],  (r, c) = T ? (x', y') : (y', x'),  x' = FX ? W-1-x : x,  y' = FY ? H-1-y : y.
// A 64 x 64 output tile therefore comes from ONE 64 x 64 source tile, whatever the element.  A workgroup copies that source
// tile into LDS with row-contiguous dword loads, and writes the output tile with row-contiguous stores, picking its bytes from
// LDS -- along a row for the mirroring elements, along a column for the transposing ones.  No lane ever walks a column of
// global memory.  LDS rows are padded by one dword to an ODD dword pitch, so the column walk (lane l on row l) lands on 32
// different banks.
#include "loft_common.h"
#include "image_prep.h"
#include "d4_tile.h"
#include "../../include/loft_hip.h"

// ---- Normalize + DefaultFormatBundle's HWC -> CHW under one element per sample -------------------------------------------------
// img uint8 [n, H, W, 3], elems int32 [n], out fp32 [n, 3, H, W].  One lane per output pixel and channel plane: a wavefront
// stores 256 contiguous bytes per plane and reads LDS at a 3-byte (mirror) or 49-dword (transpose) lane stride.
__global__ __launch_bounds__(256) void image_prep_d4_kernel(const uint8_t* __restrict__ img, const int32_t* __restrict__ elems, int H,
                                                            int W, float m0, float m1, float m2, float s0, float s1, float s2,
                                                            float* __restrict__ out) {
    __shared__ unsigned tile[D4_TILE * D4_IMG_PITCH];
    const int n = blockIdx.z, x0 = blockIdx.x * D4_TILE, y0 = blockIdx.y * D4_TILE;
    const int e = elems[n];
    // (the host has checked H == W for a transposing table, but cannot read the device table itself: a transposing entry on a
    //  non-square tile must not index past the sample, so it loses its transpose)
    const int elem = e & (H == W ? LOFT_D4_ELEMENT_MASK : LOFT_D4_ELEMENT_MASK & ~LOFT_D4_TRANSPOSE);
    const bool keep = (e & LOFT_D4_CHANNELS_KEPT) != 0;
    const D4Tile t = d4_tile(elem, H, W, x0, y0);
    // W % 4 == 0 and tile origins are multiples of 4, so every source row segment is a whole number of aligned dwords
    const unsigned* src = reinterpret_cast<const unsigned*>(img + (size_t)n * H * W * 3);
    const int rowdw = t.sw * 3 / 4;
    for (int i = threadIdx.x; i < t.sh * rowdw; i += 256) {
        const int r = i / rowdw, d = i - r * rowdw;
        tile[r * D4_IMG_PITCH + d] = src[((size_t)(t.sr0 + r) * W + t.sc0) * 3 / 4 + d];
    }
    __syncthreads();
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(tile);
    const int ox = threadIdx.x & 63;
    if (ox >= t.tw) return;
    const size_t plane = (size_t)H * W;
    const PrepNorm nm = {m0, m1, m2, s0, s1, s2};
    for (int oy = threadIdx.x >> 6; oy < t.th; oy += 4) {
        int r, c;
        d4_src(elem, t, ox, oy, r, c);
        const uint8_t* p = bytes + r * (D4_IMG_PITCH * 4) + c * 3;
        prep_store_pixel(p, keep, nm, out + (size_t)n * 3 * plane + (size_t)(y0 + oy) * W + x0 + ox, plane);
    }
}

LOFT_EXPORT int loft_image_prep_d4(const uint8_t* img, const int32_t* elems, int n, int H, int W, int any_transpose, float mean0,
                                   float mean1, float mean2, float std0, float std1, float std2, float* out, void* stream) {
    if (n < 0 || H <= 0 || W <= 0 || (W & 3) || (any_transpose && H != W) || n > 65535 || loft_cdiv(H, D4_TILE) > 65535)
        return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    if (!img || !elems || !out || ((size_t)img & 3) || ((size_t)out & 3)) return (int)hipErrorInvalidValue;
    dim3 grid(loft_cdiv(W, D4_TILE), loft_cdiv(H, D4_TILE), n);
    hipLaunchKernelGGL(image_prep_d4_kernel, grid, dim3(256), 0, (hipStream_t)stream, img, elems, H, W, mean0, mean1, mean2, std0,
                       std1, std2, out);
    LOFT_LAUNCH_CHECK();
    return 0;
}

// ---- instance bitmaps under one element ----------------------------------------------------------------------------------------
// in / out uint8 [K, H, W].  One lane per output dword (four pixels): a wavefront stores four 64-byte row segments.  A transposing
// element makes a lane read one byte from each of FOUR consecutive LDS rows, and a stride of four rows reaches only eight banks
// at any odd pitch; so every block of 32 rows is skewed by one more dword, and the two 16-lane halves of a bank group take output
// rows eight apart (two dwords apart in LDS): 4 * (g % 8) + (g / 8) + {0, 2} covers the 32 banks once.
__global__ __launch_bounds__(256) void mask_d4_kernel(const uint8_t* __restrict__ in, int elem, int H, int W, uint8_t* __restrict__ out) {
    __shared__ unsigned tile[D4_TILE * D4_MASK_PITCH + 2];
    const int k = blockIdx.z, x0 = blockIdx.x * D4_TILE, y0 = blockIdx.y * D4_TILE;
    const D4Tile t = d4_tile(elem, H, W, x0, y0);
    const unsigned* src = reinterpret_cast<const unsigned*>(in + (size_t)k * H * W);
    const int rowdw = t.sw / 4;
    for (int i = threadIdx.x; i < t.sh * rowdw; i += 256) {
        const int r = i / rowdw, d = i - r * rowdw;
        tile[mask_lds_row(r) + d] = src[((size_t)(t.sr0 + r) * W + t.sc0) / 4 + d];
    }
    __syncthreads();
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(tile);
    const int g = threadIdx.x & 15, q = threadIdx.x >> 4;
    if (4 * g >= t.tw) return;
    const int row16 = (elem & LOFT_D4_TRANSPOSE) ? (q >> 1) + 8 * (q & 1) : q;
    unsigned* dst = reinterpret_cast<unsigned*>(out + (size_t)k * H * W);
    for (int oy = row16; oy < t.th; oy += 16) {
        unsigned v = 0;
        for (int j = 0; j < 4; ++j) {
            int r, c;
            d4_src(elem, t, 4 * g + j, oy, r, c);
            v |= (unsigned)bytes[mask_lds_row(r) * 4 + c] << (8 * j);
        }
        dst[((size_t)(y0 + oy) * W + x0) / 4 + g] = v;
    }
}

LOFT_EXPORT int loft_mask_d4_u8(const uint8_t* masks, int K, int H, int W, int elem, uint8_t* out, void* stream) {
    if (K < 0 || H <= 0 || W <= 0 || (W & 3) || (elem & ~LOFT_D4_ELEMENT_MASK) || ((elem & LOFT_D4_TRANSPOSE) && H != W) ||
        K > 65535 || loft_cdiv(H, D4_TILE) > 65535)
        return (int)hipErrorInvalidValue;
    if (K == 0) return 0;
    if (!masks || !out || masks == out || ((size_t)masks & 3) || ((size_t)out & 3)) return (int)hipErrorInvalidValue;
    dim3 grid(loft_cdiv(W, D4_TILE), loft_cdiv(H, D4_TILE), K);
    hipLaunchKernelGGL(mask_d4_kernel, grid, dim3(256), 0, (hipStream_t)stream, masks, elem, H, W, out);
    LOFT_LAUNCH_CHECK();
    return 0;
}
