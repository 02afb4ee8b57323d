// Tile constants and host arithmetic of the gather kernels (vp_remap.hip): cv2.remap, cv2.convertMaps and cv2.warpPerspective.
// Plain C++ - no HIP types, no kernels - and pure functions of their arguments, like vp_deriv_plan.h.
#pragma once

// the tile of k_remap_fixed, k_remap_f32 and k_warp_perspective: one wave per destination row, RM_PPT adjacent pixels per lane
#define RM_PPT 4               // destination pixels per lane: 16 bytes of int16 x,y map, 8 of fractions, 4 * cn bytes stored at once
#define RM_TW 256              // destination pixels per tile row: 64 lanes x RM_PPT
#define RM_TH 4                // destination rows per tile (256 threads)
#define RM_MAX_SRC 32767       // cv2 asserts the source fits int16 coordinates
#define RM_MAX_ROWS 65535      // destination rows, as the other operators
#define RM_MAX_COLS (1 << 24)  // destination columns
#define RM_CVT_BLOCK 256       // k_convert_maps: one map entry per thread

// cv::WarpPerspectiveInvoker's block width (BLOCK_SZ = 32): columns [bx, bx + bw0) share the products M0 bx, M3 bx, M6 bx
static inline int vp_wp_block_width(int dst_w, int dst_h)
{
    const int bh0 = dst_h < 16 ? dst_h : 16;
    const int q = 1024 / bh0;
    return q < dst_w ? q : dst_w;
}

// launch geometry of the tile kernels: blocks of (64, RM_TH) threads
static inline unsigned vp_remap_grid_x(int w) { return (unsigned)((w + RM_TW - 1) / RM_TW); }
static inline unsigned vp_remap_grid_y(int h) { return (unsigned)((h + RM_TH - 1) / RM_TH); }

// a map (= destination) the grids cover: k_convert_maps runs one thread per entry in a 1-D grid, so the entry count is bounded too
#define RM_MAX_ENTRIES (1ll << 31)
static inline int vp_remap_map_ok(int mw, int mh)
{
    return mw > 0 && mh > 0 && mw <= RM_MAX_COLS && mh <= RM_MAX_ROWS && (long long)mw * mh < RM_MAX_ENTRIES;
}

// the sizes every entry accepts: a source cv2 accepts, a destination the grid covers
static inline int vp_remap_sizes_ok(int sw, int sh, int cn, int dw, int dh)
{
    return sw > 0 && sh > 0 && sw <= RM_MAX_SRC && sh <= RM_MAX_SRC && cn >= 1 && cn <= 4 && vp_remap_map_ok(dw, dh);
}
