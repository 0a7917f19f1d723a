// box_codec.h -- the per-row arithmetic of the box / offset coders and of the mask paste, as __device__ functions: boxes.hip's
// kernels and the test-time-augmentation merges of tta.hip call the SAME code (one statement of each formula; both files are built
// with -ffp-contract=off, so a row decodes to the same bits in either).
#pragma once
#include "loft_common.h"
#include "../../include/loft_hip.h"

// ---- DeltaXYWHBBoxCoder.decode (delta_xywh_bbox_coder.py:118-204) ------------------------------------------------------------------
__device__ __forceinline__ float4 decode_box(const float4 r, float d0, float d1, float d2, float d3, const float* means,
                                             const float* stds, float max_ratio, float max_h, float max_w) {
    const float dx = d0 * stds[0] + means[0], dy = d1 * stds[1] + means[1];
    float dw = d2 * stds[2] + means[2], dh = d3 * stds[3] + means[3];
    dw = fminf(fmaxf(dw, -max_ratio), max_ratio);
    dh = fminf(fmaxf(dh, -max_ratio), max_ratio);
    const float px = (r.x + r.z) * 0.5f, py = (r.y + r.w) * 0.5f;
    const float pw = r.z - r.x, ph = r.w - r.y;
    const float gw = pw * expf(dw), gh = ph * expf(dh);
    const float gx = px + pw * dx, gy = py + ph * dy;
    float4 o;
    o.x = gx - gw * 0.5f; o.y = gy - gh * 0.5f; o.z = gx + gw * 0.5f; o.w = gy + gh * 0.5f;
    if (max_w > 0.f) {
        o.x = fminf(fmaxf(o.x, 0.f), max_w); o.z = fminf(fmaxf(o.z, 0.f), max_w);
        o.y = fminf(fmaxf(o.y, 0.f), max_h); o.w = fminf(fmaxf(o.w, 0.f), max_h);
    }
    return o;
}

struct Coder4 { float means[4], stds[4]; };

// ---- FOA fusion + decode of one RoI: pred [4n,2] branch-major, row i (offset_head_expand_feature.py:346-448) -------------------------
__device__ __forceinline__ float2 foa_fuse_decode_one(const float* __restrict__ pred, long n, long i, const float4 r, float std_x,
                                                      float std_y, float max_h, float max_w) {
    const float b0x = pred[(0 * n + i) * 2], b0y = pred[(0 * n + i) * 2 + 1];
    const float b1x = pred[(1 * n + i) * 2], b1y = pred[(1 * n + i) * 2 + 1];
    const float b2x = pred[(2 * n + i) * 2], b2y = pred[(2 * n + i) * 2 + 1];
    const float b3x = pred[(3 * n + i) * 2], b3y = pred[(3 * n + i) * 2 + 1];
    const float vx = fmaxf(fmaxf(fabsf(b0x), fabsf(b1y)), fmaxf(fabsf(b2x), fabsf(b3y)));
    const float vy = fmaxf(fmaxf(fabsf(b0y), fabsf(b1x)), fmaxf(fabsf(b2y), fabsf(b3x)));
    const float fx = vx * (b0x > 0.f ? 1.f : -1.f), fy = vy * (b0y > 0.f ? 1.f : -1.f);
    float gx = (r.z - r.x) * (fx * std_x), gy = (r.w - r.y) * (fy * std_y);
    gx = fminf(fmaxf(gx, -max_w), max_w);
    gy = fminf(fmaxf(gy, -max_h), max_h);
    return make_float2(gx, gy);
}

// ---- plain OffsetHead decode of one RoI: pred [n,reg_num], row i (offset_head.py:190-243) ---------------------------------------------
__device__ __forceinline__ float2 offset_decode_one(const float* __restrict__ pred, long i, const float4 r, float mean_x, float mean_y,
                                                    float std_x, float std_y, float max_h, float max_w, int reg_num, int polar) {
    float d0, d1;
    if (reg_num == 2) { d0 = pred[2 * i]; d1 = pred[2 * i + 1]; }
    else { d0 = pred[3 * i]; d1 = atan2f(pred[3 * i + 2], pred[3 * i + 1]); }
    float gx = (r.z - r.x) * (d0 * std_x + mean_x), gy = (r.w - r.y) * (d1 * std_y + mean_y);
    gx = fminf(fmaxf(gx, -max_w), max_w);
    gy = fminf(fmaxf(gy, -max_h), max_h);
    if (polar) { const float l = gx, a = gy; gx = l * cosf(a); gy = l * sinf(a); }
    return make_float2(gx, gy);
}

// ---- mask paste of one output pixel (_do_paste_mask, fcn_mask_head.py:240-308) --------------------------------------------------------
// the reference's CPU path (skip_empty=True, one instance per chunk) samples only the tight integer region around the box
__device__ __forceinline__ bool paste_outside(int x, int y, const float4 b, int img_h, int img_w) {
    return (float)x < fmaxf(floorf(b.x) - 1.f, 0.f) || (float)x >= fminf(ceilf(b.z) + 1.f, (float)img_w) ||
           (float)y < fmaxf(floorf(b.y) - 1.f, 0.f) || (float)y >= fminf(ceilf(b.w) + 1.f, (float)img_h);
}
// the pixels paste_outside does not exclude, as the integer window [x0, x1) x [y0, y1) (its bounds are whole numbers); empty when
// x0 >= x1 or y0 >= y1
struct PasteWin { int x0, x1, y0, y1; };
__device__ __forceinline__ PasteWin paste_window(const float4 b, int img_h, int img_w) {
    const float fw = (float)img_w, fh = (float)img_h;
    PasteWin w;
    w.x0 = (int)fminf(fmaxf(floorf(b.x) - 1.f, 0.f), fw);
    w.x1 = (int)fmaxf(fminf(ceilf(b.z) + 1.f, fw), 0.f);
    w.y0 = (int)fminf(fmaxf(floorf(b.y) - 1.f, 0.f), fh);
    w.y1 = (int)fmaxf(fminf(ceilf(b.w) + 1.f, fh), 0.f);
    return w;
}
// bilinear grid_sample(align_corners=False, zero padding) of the S x S probabilities at pixel (x, y); at(yy, xx) gives one tap's
// probability, 0 outside the grid
template <typename At>
__device__ __forceinline__ float paste_sample(int x, int y, const float4 b, int S, At at) {
    float gx = ((float)x + 0.5f - b.x) / (b.z - b.x) * 2.f - 1.f;
    float gy = ((float)y + 0.5f - b.y) / (b.w - b.y) * 2.f - 1.f;
    if (isinf(gx)) gx = 0.f;
    if (isinf(gy)) gy = 0.f;
    // grid_sample, align_corners=False: source coordinate = ((g + 1) * S - 1) / 2
    const float sx = ((gx + 1.f) * (float)S - 1.f) * 0.5f, sy = ((gy + 1.f) * (float)S - 1.f) * 0.5f;
    float v = 0.f;
    if (sx > -1.f && sx < (float)S && sy > -1.f && sy < (float)S) {
        const float fx = floorf(sx), fy = floorf(sy);
        const int x0 = (int)fx, y0 = (int)fy;
        const float lx = sx - fx, ly = sy - fy;
        v = at(y0, x0) * (1.f - ly) * (1.f - lx) + at(y0, x0 + 1) * (1.f - ly) * lx + at(y0 + 1, x0) * ly * (1.f - lx) +
            at(y0 + 1, x0 + 1) * ly * lx;
    }
    return v;
}
__device__ __forceinline__ float paste_sigmoid(float logit) { return 1.f / (1.f + expf(-logit)); }
// the merged taps of one detection, staged by the whole workgroup (aug_test_mask + merge_aug_masks, test_mixins.py:179-208): tap
// (r, c) = the sequential fp32 sum, in view order, of sigmoid(logit) read through each view's inverse permutation of the S x S grid
// (LOFT_D4_*: original tap (r, c) is the view's tap (y, x), (y', x') = T ? (c, r) : (r, c), then the mirrors), divided by V.
// logits [V,N,S,S]; taps: S*S floats of LDS; the caller synchronises before reading them.  V == 1 with the identity element
// leaves paste_sigmoid(logit), bit for bit.
__device__ __forceinline__ void paste_stage_taps(float* taps, const float* __restrict__ logits, int n, int N, int V, int S,
                                                 const int32_t* __restrict__ views) {
    const int SS = S * S;
    for (int k = threadIdx.x; k < SS; k += blockDim.x) {
        const int r = k / S, c = k - r * S;
        float acc = 0.f;
        for (int v = 0; v < V; ++v) {
            const int e = views[v] & LOFT_D4_ELEMENT_MASK;
            int yv = (e & LOFT_D4_TRANSPOSE) ? c : r, xv = (e & LOFT_D4_TRANSPOSE) ? r : c;
            if (e & LOFT_D4_MIRROR_X) xv = S - 1 - xv;
            if (e & LOFT_D4_MIRROR_Y) yv = S - 1 - yv;
            acc += paste_sigmoid(logits[((long)v * N + n) * SS + yv * S + xv]);
        }
        taps[k] = acc / (float)V;
    }
}
