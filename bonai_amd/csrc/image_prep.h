// image_prep.h -- Normalize + DefaultFormatBundle's HWC -> CHW of ONE pixel, as a __device__ function: augment.hip's
// loft_image_prep_d4 and scene.hip's loft_scene_tile_prep call the SAME statement (both files are built with -ffp-contract=off:
// an IEEE subtract followed by an IEEE divide, bit for bit the torch chain of data.to_device_batch).
#pragma once
#include "loft_common.h"

struct PrepNorm { float m0, m1, m2, s0, s1, s2; };

// p: the pixel's three source bytes; keep: channel c of the output is channel c of the input (else reversed, Normalize's to_rgb);
// o: the pixel's place in the first output plane, the planes `plane` floats apart
__device__ __forceinline__ void prep_store_pixel(const uint8_t* p, bool keep, const PrepNorm& nm, float* o, size_t plane) {
    const float v0 = (float)p[keep ? 0 : 2], v1 = (float)p[1], v2 = (float)p[keep ? 2 : 0];
    o[0] = (v0 - nm.m0) / nm.s0;
    o[plane] = (v1 - nm.m1) / nm.s1;
    o[2 * plane] = (v2 - nm.m2) / nm.s2;
}
