// How many persistent work-groups the convolution kernels launch, and how those of the 3x3 kernels (conv3x3_wide.hip,
// conv3x3_stream.hip) walk their tile list: plain static stride, or one contiguous band of the list per XCD.
#pragma once
#include "mas_common.h"

// MAS_CONV_XCD_BANDS (default 1; 0 = the plain maps, for A/B runs), read once per process
static inline bool mas_xcd_bands_enabled() {
    static const int bands = mas_env_int("MAS_CONV_XCD_BANDS", 1);
    return bands != 0;
}
// Work-groups of a persistent grid: per_cu on every CU (the caller's default; MAS_CONV_WGS_PER_CU = n > 0, read once per process,
// overrides it -- tests: one work-group per CU -> several tiles per work-group).  The grid is min(tiles, this).
static inline long long mas_resident_wgs(int per_cu) {
    static const int wgs_per_cu = mas_env_int("MAS_CONV_WGS_PER_CU", 0);
    return (long long)(wgs_per_cu > 0 ? wgs_per_cu : per_cu) * mas_num_cus();
}
// May a launch of `blocks` work-groups over `tiles` tiles take the banded walk?  It needs a grid that is a multiple of the 8 XCDs and
// every band at least as long as the number of work-groups that walk it.
static inline bool mas_xcd_band_walk_ok(long long blocks, long long tiles) {
    return mas_xcd_bands_enabled() && blocks % 8 == 0 && tiles / 8 >= blocks / 8;
}

// Tile walk of this work-group (blockIdx.x of a gridDim.x <= total_tiles): it takes tile, tile + step, ... below tile_end.
// (The two indices are read here, not passed in: as arguments they change the instruction selection of the callers' prologues.)
// Work-group b runs on XCD b % 8 (observed dispatch order; speed only, never correctness).  With the plain static stride
// (b, b + G, ...) the 32 CUs of an XCD work on tiles 8 apart: no two of them share a halo, and every 18x34 patch (1.195x its tile)
// comes over the fabric.  xcd_bands: XCD x owns the contiguous eighth [T x / 8, T (x + 1) / 8) of the tile list and its work-groups
// walk it in order, so the tiles in flight on one XCD are spatial neighbours (a whole image of a 256^2 map; the cout tiles that share a
// patch are consecutive tile ids) and their halos meet in that XCD's L2 (profiles/r06_xcd_bands.txt).  Same registers as the plain
// walk: `step` stands where gridDim.x stood, `tile_end` where total_tiles did.
__device__ __forceinline__ void xcd_band_walk(int total_tiles, int xcd_bands, int& tile, int& step, int& tile_end) {
    tile = blockIdx.x;
    step = (int)gridDim.x; tile_end = total_tiles;
    if (xcd_bands && (gridDim.x & 7) == 0) {
        const int x = blockIdx.x & 7;
        step = (int)(gridDim.x >> 3);
        tile = (int)(((long long)total_tiles * x) >> 3) + (int)(blockIdx.x >> 3);
        tile_end = (int)(((long long)total_tiles * (x + 1)) >> 3);
    }
}
