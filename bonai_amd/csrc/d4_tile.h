// d4_tile.h -- the 64 x 64 tile geometry of the square's eight symmetries, shared by augment.hip (permutation alone) and resize.hip
// (Resize in front of it): which source tile an output tile comes from, and where an output pixel sits inside that tile in LDS.
#pragma once
#include "loft_common.h"
#include "../../include/loft_hip.h"

#define D4_TILE 64
#define D4_IMG_PITCH (D4_TILE * 3 / 4 + 1)      // dwords per LDS row of the image tile: 48 of pixels + 1 of padding = 49 (odd)
#define D4_MASK_PITCH (D4_TILE / 4 + 1)         // dwords per LDS row of the bitmap tile: 16 + 1 = 17 (odd)

struct D4Tile {            // the source tile of one output tile
    int tw, th;            // extent of the output tile (partial at the right / bottom edge)
    int sr0, sc0;          // first source row / column
    int sh, sw;            // source rows / columns
};

__device__ __forceinline__ D4Tile d4_tile(int elem, int H, int W, int x0, int y0) {
    D4Tile t;
    t.tw = min(D4_TILE, W - x0);
    t.th = min(D4_TILE, H - y0);
    const int mx0 = (elem & LOFT_D4_MIRROR_X) ? W - x0 - t.tw : x0;      // where the tile's x' and y' ranges start
    const int my0 = (elem & LOFT_D4_MIRROR_Y) ? H - y0 - t.th : y0;
    if (elem & LOFT_D4_TRANSPOSE) { t.sr0 = mx0; t.sh = t.tw; t.sc0 = my0; t.sw = t.th; }
    else                          { t.sr0 = my0; t.sh = t.th; t.sc0 = mx0; t.sw = t.tw; }
    return t;
}

// (row, column) inside the LDS tile of output pixel (ox, oy) of the tile
__device__ __forceinline__ void d4_src(int elem, const D4Tile& t, int ox, int oy, int& r, int& c) {
    const int lx = (elem & LOFT_D4_MIRROR_X) ? t.tw - 1 - ox : ox;
    const int ly = (elem & LOFT_D4_MIRROR_Y) ? t.th - 1 - oy : oy;
    r = (elem & LOFT_D4_TRANSPOSE) ? lx : ly;
    c = (elem & LOFT_D4_TRANSPOSE) ? ly : lx;
}

// dword index of row r of the bitmap tile in LDS: every block of 32 rows skewed by one more dword (augment.hip says why)
__device__ __forceinline__ int mask_lds_row(int r) { return r * D4_MASK_PITCH + (r >> 5); }

