// Host arithmetic of cv2.distanceTransform and cv2.minMaxLoc (vp_dist.hip): the argument checks as this library admits them, the
// bounds that keep every distance an exact integer, the launch geometry, the choice between the two forms of the column pass with
// its LDS budget, and the 64-bit keys of the minimum / maximum search.  Plain C++ - no HIP types, no kernels - and a pure function of
// its arguments, like vp_corners_plan.h, whose order-preserving float key the search reuses.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "vp_corners_plan.h"

// metrics (cv2's DIST_* values) and the admitted sizes
#define DT_METRIC_L1 1
#define DT_METRIC_L2 2
#define DT_METRIC_C 3
#define DT_MAX_SIDE 4096       // rows and columns: a row is at most 64 words of 64 bits, one per lane of a wave
#define DT_NONE 16384          // g of a pixel whose row holds no zero; a column minimum at or above its cost is "no zero in the image"

// the row pass: one wave per row, DT_ROW_WAVES rows per block; g rows are padded to whole words of 64 pixels
#define DT_ROW_WAVES 4
// the column pass: 256 threads, four neighbouring pixels of a row per lane (one 8-byte read of g, one 16-byte float store)
#define DT_PX 4
#define DT_LDS_BYTES 65536     // static LDS a block of this library may use
#define DT_STRIP_COLS 16       // staged form: columns of g a block keeps in LDS, all h rows of them
#define DT_STRIP_ROWS 128      // ... and the result rows it computes from them
#define DT_WIDE_COLS 64        // direct form: columns per block, g read from device memory
#define DT_WIDE_ROWS 64
#define DT_STAGED_MAX_H (DT_LDS_BYTES / (DT_STRIP_COLS * 2))     // 2048: the tallest image whose strip of uint16 columns fits
#define DT_SWITCH_H (DT_STAGED_MAX_H + 1)                        // the first height the direct form takes

static_assert(DT_MAX_SIDE == 64 * 64, "distance transform: a row is one wave of 64-bit words");
static_assert(DT_STAGED_MAX_H * DT_STRIP_COLS * 2 <= DT_LDS_BYTES, "distance transform: the staged strip above 64 KiB of LDS");
static_assert(DT_STRIP_COLS % DT_PX == 0 && DT_WIDE_COLS % DT_PX == 0 && 256 % (DT_STRIP_COLS / DT_PX) == 0 && 256 % (DT_WIDE_COLS / DT_PX) == 0,
              "distance transform: whole rows of lanes per block");
static_assert(DT_STRIP_ROWS % (256 / (DT_STRIP_COLS / DT_PX)) == 0 && DT_WIDE_ROWS % (256 / (DT_WIDE_COLS / DT_PX)) == 0,
              "distance transform: whole passes per block");
// every true distance is below the cost of DT_NONE, and every cost fits int32: dx^2 + dy^2 <= 2 * 4095^2 < DT_NONE^2, DT_NONE^2 + 4095^2 < 2^31
static_assert(2ll * (DT_MAX_SIDE - 1) * (DT_MAX_SIDE - 1) < (long long)DT_NONE * DT_NONE, "distance transform: a squared distance reaches the sentinel");
static_assert((long long)DT_NONE * DT_NONE + (long long)(DT_MAX_SIDE - 1) * (DT_MAX_SIDE - 1) < (1ll << 31), "distance transform: a cost above int32");
static_assert(2 * (DT_MAX_SIDE - 1) < DT_NONE && 2 * (DT_MAX_SIDE - 1) < 8192, "distance transform: an L1 distance reaches the sentinel or cv2's clamp");
static_assert((long long)(DT_MAX_SIDE - 1) * (DT_MAX_SIDE - 1) < (1ll << 24), "distance transform: dx^2 is not exact in float32");
static_assert((long long)DT_MAX_SIDE * DT_MAX_SIDE <= (1ll << 24), "min / max search: the raster index above 2^24");

// 1: the strip of columns staged in LDS; 0: g read from device memory (h above what the LDS budget holds)
static inline int vp_dist_staged(int h) { return h < DT_SWITCH_H; }
static inline size_t vp_dist_lds_bytes(int h) { return vp_dist_staged(h) ? (size_t)h * DT_STRIP_COLS * 2 : 0; }
static inline int vp_dist_g_pitch(int w) { return (w + 63) / 64 * 64; }                    // uint16 elements per row of g
static inline size_t vp_dist_g_bytes(int w, int h) { return (size_t)vp_dist_g_pitch(w) * h * 2; }
static inline void vp_dist_grid(int w, int h, unsigned* gx, unsigned* gy)
{
    const int cols = vp_dist_staged(h) ? DT_STRIP_COLS : DT_WIDE_COLS, rows = vp_dist_staged(h) ? DT_STRIP_ROWS : DT_WIDE_ROWS;
    *gx = (unsigned)((w + cols - 1) / cols);
    *gy = (unsigned)((h + rows - 1) / rows);
}

// depths as VP_DEPTH_8U / VP_DEPTH_32F of vp.h
#define DT_DEPTH_8U 0
#define DT_DEPTH_32F 5

// NULL: admitted; else the reason (VP_ERR_INVALID).  dst_stride in bytes.
static inline const char* vp_distance_transform_refusal(int w, int h, size_t stride, int has_src, int has_bits, int metric, int dst_depth, size_t dst_stride)
{
    if (has_bits && !has_src) return "distance transform: a bit plane without its source image";
    if (w < 1 || h < 1) return "distance transform: width and height must be at least 1";
    if (w > DT_MAX_SIDE || h > DT_MAX_SIDE) return "distance transform: width and height must be at most 4096";
    if (stride < (size_t)w) return "distance transform: the stride is below the row";
    if (metric != DT_METRIC_L1 && metric != DT_METRIC_L2 && metric != DT_METRIC_C) return "distance transform: the metric must be DIST_L1, DIST_L2 or DIST_C";
    if (dst_depth != DT_DEPTH_8U && dst_depth != DT_DEPTH_32F) return "distance transform: the result must be CV_8U or CV_32F";
    if (dst_depth == DT_DEPTH_8U && metric != DT_METRIC_L1) return "distance transform: a CV_8U result only with DIST_L1";
    const size_t es = dst_depth == DT_DEPTH_8U ? 1 : 4;
    if (dst_stride < (size_t)w * es) return "distance transform: the result's stride is below the row";
    if (dst_stride % es) return "distance transform: the result's stride is not a multiple of the element size";
    return nullptr;
}

// stride and mask_stride in bytes
static inline const char* vp_min_max_loc_refusal(int w, int h, size_t stride, int depth, int has_mask, int mask_w, int mask_h, size_t mask_stride)
{
    if (w < 1 || h < 1) return "min max loc: width and height must be at least 1";
    if (w > DT_MAX_SIDE || h > DT_MAX_SIDE) return "min max loc: width and height must be at most 4096";
    if (depth != DT_DEPTH_8U && depth != DT_DEPTH_32F) return "min max loc: the depth must be 8U or 32F";
    const size_t es = depth == DT_DEPTH_8U ? 1 : 4;
    if (stride < (size_t)w * es) return "min max loc: the stride is below the row";
    if (stride % es) return "min max loc: the stride is not a multiple of the element size";
    if (has_mask && (mask_w != w || mask_h != h)) return "min max loc: the mask must have the size of the image";
    if (has_mask && mask_stride < (size_t)w) return "min max loc: the mask's stride is below the row";
    return nullptr;
}

// The two ends of the search are 64-bit maxima: the order-preserving key of the value (complemented for the minimum) in the high half,
// 2^32 - 1 - raster index in the low half, so that among equal values the smallest raster index wins at both ends.  The index is at
// most 2^24, so the low half is never 0 and the word 0 means "no pixel took part".
VP_CORNERS_HD static inline unsigned long long vp_mml_key(uint32_t float_bits, uint32_t index, int minimum)
{
    const uint32_t k = vp_corner_key(float_bits);
    return ((unsigned long long)(minimum ? ~k : k) << 32) | (0xffffffffu - index);
}
VP_CORNERS_HD static inline uint32_t vp_mml_value_bits(unsigned long long key, int minimum)
{
    const uint32_t k = (uint32_t)(key >> 32);
    return vp_corner_unkey(minimum ? ~k : k);
}
VP_CORNERS_HD static inline uint32_t vp_mml_index(unsigned long long key) { return 0xffffffffu - (uint32_t)key; }

// what vp_min_max_loc_* write: cv2.minMaxLoc's four results
struct vp_min_max_loc_result { double min_val, max_val; int min_x, min_y, max_x, max_y; };

// the two words of the device search -> the result; an empty search gives (0, 0, (-1, -1), (-1, -1))
static inline void vp_min_max_loc_decode(unsigned long long kmin, unsigned long long kmax, int w, vp_min_max_loc_result* out)
{
    out->min_val = out->max_val = 0.0;
    out->min_x = out->min_y = out->max_x = out->max_y = -1;
    if (kmin == 0 || kmax == 0) return;
    union { uint32_t u; float f; } a, b;
    a.u = vp_mml_value_bits(kmin, 1);
    b.u = vp_mml_value_bits(kmax, 0);
    const uint32_t imin = vp_mml_index(kmin), imax = vp_mml_index(kmax);
    out->min_val = (double)a.f;
    out->max_val = (double)b.f;
    out->min_y = (int)(imin / (uint32_t)w);
    out->min_x = (int)(imin - (uint32_t)out->min_y * (uint32_t)w);
    out->max_y = (int)(imax / (uint32_t)w);
    out->max_x = (int)(imax - (uint32_t)out->max_y * (uint32_t)w);
}
