// Host arithmetic of the corner operators (vp_corners.hip): the argument checks of cv2.cornerMinEigenVal / cornerHarris /
// goodFeaturesToTrack as this library admits them, the tile of the response kernel, the bound that keeps the structure tensor in
// int32, the launch geometry, and the greedy minDistance pass, which runs on the host.  Plain C++ - no HIP types, no kernels - and a
// pure function of its arguments, like vp_deriv_plan.h, whose border index map the kernels reuse.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "vp_deriv_plan.h"

// the tile of the response kernel (the kernel asserts its LDS budget from the same numbers)
#define CR_TW 64               // result columns per tile: one wave per result row group
#define CR_TH 16               // result rows per tile
#define CR_SEG 16              // results one thread slides its row sum over
#define CR_MAX_BLOCK 31        // largest blockSize
#define CR_MAX_DERIV 1020      // |Dx|, |Dy| of the 3x3 Sobel on uint8: 4 * 255
#define CR_MAX_SIDE 65535      // rows and columns
#define CR_MAX_PIXELS 268435456   // 2^28: a raster index and a candidate count fit 32 bits with room

// every box sum of products fits int32: the statement test repeats this for every admitted blockSize
static_assert((long long)CR_MAX_BLOCK * CR_MAX_BLOCK * CR_MAX_DERIV * CR_MAX_DERIV < (1ll << 31), "corner response: a box sum of products above int32");
static_assert(CR_TW == 64 && CR_TH % 4 == 0 && CR_TW % CR_SEG == 0, "corner response: 64 columns per wave, four row groups per tile");

// the kernel instantiations: the largest blockSize each one's LDS planes hold
static inline int vp_corner_block_class(int block_size) { return block_size <= 3 ? 3 : block_size <= 7 ? 7 : CR_MAX_BLOCK; }

// NULL: admitted; else the reason (VP_ERR_INVALID)
static inline const char* vp_corner_response_refusal(int w, int h, size_t stride, int block_size, int ksize, double k, int border)
{
    if (w < 1 || h < 1) return "corner response: width and height must be at least 1";
    if (w > CR_MAX_SIDE || h > CR_MAX_SIDE) return "corner response: width and height must be at most 65535";
    if ((long long)w * h > CR_MAX_PIXELS) return "corner response: more than 2^28 pixels";
    if (stride < (size_t)w) return "corner response: the stride is below the row";
    if (block_size < 1 || block_size > CR_MAX_BLOCK) return "corner response: blockSize must be in 1..31";
    if (ksize != 3) return "corner response: only ksize 3 (the 3x3 Sobel) is restated";
    if (!isfinite(k)) return "corner response: k must be finite";
    const int b = border & ~VP_DV_ISOLATED;
    if (b != VP_DV_CONSTANT && b != VP_DV_REPLICATE && b != VP_DV_REFLECT && b != VP_DV_REFLECT_101)
        return "corner response: the border must be REFLECT_101, REPLICATE, REFLECT or CONSTANT";
    return nullptr;
}

static inline const char* vp_good_features_refusal(int w, int h, size_t stride, double quality, double min_distance, int has_mask, int mask_w, int mask_h,
                                                   size_t mask_stride, int block_size, double k, int capacity)
{
    if (const char* why = vp_corner_response_refusal(w, h, stride, block_size, 3, k, VP_DV_REFLECT_101)) return why;
    if (!(quality > 0) || !isfinite(quality)) return "good features: qualityLevel must be positive and finite";
    if (!(min_distance >= 0)) return "good features: minDistance must be at least 0";
    if (capacity < 0) return "good features: the capacity is negative";
    if (has_mask && (mask_w != w || mask_h != h)) return "good features: the mask must have the size of the image";
    if (has_mask && mask_stride < (size_t)w) return "good features: the mask's stride is below the row";
    return nullptr;
}

// s = 1 / (4 * blockSize * 255): the scale cornerEigenValsVecs gives the Sobel of a uint8 image
static inline double vp_corner_scale(int block_size) { return 1.0 / (4.0 * block_size * 255.0); }

// The order-preserving map of float32 bit patterns to unsigned integers (a > b as floats <=> key(a) > key(b); -0 sorts below +0, which
// no comparison here can see): the maximum is an integer atomic and a candidate's key sorts as an integer.  0 is below every key.
#ifdef __HIPCC__
#define VP_CORNERS_HD __host__ __device__
#else
#define VP_CORNERS_HD
#endif
VP_CORNERS_HD static inline uint32_t vp_corner_key(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
VP_CORNERS_HD static inline uint32_t vp_corner_unkey(uint32_t key) { return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key; }

// Candidates arrive as 64-bit words sorted ascending, word = ~(key(resp) << 32 | raster index): strongest first, equal responses by
// larger raster index first (OpenCV's greaterThanPtr).  The greedy pass of goodFeaturesToTrack over the first n of them: a candidate
// is kept unless a kept corner lies at dx * dx + dy * dy < minDistance^2, until max_corners > 0 are kept.  Integer coordinates, so the
// test is exact; kept corners hang off a grid of cells of at least minDistance pixels, and only the 3 x 3 cells round a candidate are
// searched, as featureselect.cpp does.  Two pixels are at least 1 apart, so minDistance <= 1 drops nothing.  Writes the first
// `capacity` (x, y) pairs and returns the number kept.
static inline long long vp_good_features_select(const unsigned long long* sorted, long long n, int w, int h, int max_corners, double min_distance, float* out_xy,
                                                long long capacity)
{
    const double md2 = min_distance * min_distance;
    const bool spaced = md2 > 1.0;
    int cell = 1, gw = 0, gh = 0;
    std::vector<int32_t> head, next;
    std::vector<uint32_t> kept;
    if (spaced) {
        const double c = ceil(min_distance);
        cell = c >= (double)CR_MAX_SIDE ? CR_MAX_SIDE + 1 : (int)c;
        gw = (w + cell - 1) / cell;
        gh = (h + cell - 1) / cell;
        head.assign((size_t)gw * gh, -1);
    }
    long long nk = 0;
    for (long long i = 0; i < n; i++) {
        const uint32_t idx = (uint32_t)~sorted[i];
        const int y = (int)(idx / (uint32_t)w), x = (int)(idx - (uint32_t)y * (uint32_t)w);
        if (spaced) {
            const int cx = x / cell, cy = y / cell;
            bool close = false;
            for (int yy = cy > 0 ? cy - 1 : 0; yy <= cy + 1 && yy < gh && !close; yy++)
                for (int xx = cx > 0 ? cx - 1 : 0; xx <= cx + 1 && xx < gw && !close; xx++)
                    for (int32_t q = head[(size_t)yy * gw + xx]; q >= 0; q = next[q]) {
                        const long long dx = x - (int)(kept[q] & 0xffffu), dy = y - (int)(kept[q] >> 16);
                        if ((double)(dx * dx + dy * dy) < md2) { close = true; break; }
                    }
            if (close) continue;
            kept.push_back((uint32_t)x | ((uint32_t)y << 16));
            next.push_back(head[(size_t)cy * gw + cx]);
            head[(size_t)cy * gw + cx] = (int32_t)nk;
        }
        if (nk < capacity) {
            out_xy[2 * nk] = (float)x;
            out_xy[2 * nk + 1] = (float)y;
        }
        nk++;
        if (max_corners > 0 && nk == max_corners) break;
    }
    return nk;
}
