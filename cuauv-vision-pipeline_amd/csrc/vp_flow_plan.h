// Host arithmetic of cv2.calcOpticalFlowPyrLK (vp_flow.hip): the argument checks as this library admits them, the rule that says
// which pyramid levels exist, the level sizes, the index reflection every image read goes through, the LDS layout of one point and
// the grid.  Plain C++ - no HIP types, no kernels - and a pure function of its arguments, like vp_hist_plan.h.  DESIGN.md section
// 4.29; tests/flow_restate.py is the statement.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define VP_FLOW_HD __host__ __device__
#else
#define VP_FLOW_HD
#endif

#define LK_MAX_SIDE 4096         // rows and columns of level 0
#define LK_MIN_WIN 3             // a window side
#define LK_MAX_WIN 63
#define LK_MAX_LEVELS 16         // max_level 0..15
#define LK_MAX_POINTS (1 << 20)
#define LK_MAX_COUNT 100         // iterations per level (cv2 clamps its TermCriteria the same way)
#define LK_MAX_EPS 10.0
#define LK_COORD_LIMIT 16777216.0f   // 2^24: a coordinate beyond it (or not finite) is never converted to an integer
#define LK_LANES 64              // one wave per point: every barrier of the kernel is uniform by construction
#define LK_LDS_BYTES 163840      // what a gfx950 workgroup may take
#define LK_W_BITS 14

#define LK_USE_INITIAL_FLOW 4    // cv2.OPTFLOW_USE_INITIAL_FLOW
#define LK_GET_MIN_EIGENVALS 8   // cv2.OPTFLOW_LK_GET_MIN_EIGENVALS

// the levels of both pyramids as the kernel receives them, in one argument block
struct vp_lk_levels {
    const uint8_t* prev[LK_MAX_LEVELS];
    const uint8_t* next[LK_MAX_LEVELS];
    size_t prev_stride[LK_MAX_LEVELS];
    size_t next_stride[LK_MAX_LEVELS];
    int32_t cols[LK_MAX_LEVELS];
    int32_t rows[LK_MAX_LEVELS];
};

struct vp_lk_plan {
    int levels;                  // existing levels at or below the requested one, at least 1: the effective maxLevel is levels - 1
    int cols[LK_MAX_LEVELS], rows[LK_MAX_LEVELS];
    int patch_w, patch_h;        // the window, +1 for the bilinear neighbour, +1 on each side for the Scharr taps
    size_t off_deriv, off_win;   // LDS of one point: patch bytes | (ww + 1)(wh + 1) int16 pairs (Ix, Iy) | three planes of ww wh int16: I, Ix, Iy
    size_t lds_bytes;
    unsigned grid;               // one workgroup of LK_LANES per point
};

static inline int vp_lk_half(int v) { return (v + 1) / 2; }     // a side of pyrDown's result

// levels 0 .. max_level that exist: level l exists while its width is above win_w and its height above win_h; 0 when level 0 does not
static inline int vp_lk_level_count(int w, int h, int win_w, int win_h, int max_level)
{
    int n = 0;
    while (n <= max_level && n < LK_MAX_LEVELS && w > win_w && h > win_h) {
        n++;
        w = vp_lk_half(w);
        h = vp_lk_half(h);
    }
    return n;
}

// BORDER_REFLECT_101 of index i on a line of n >= 2 pixels, then clamped: whatever i is, the result is inside 0 .. n - 1.  The level
// rule (n > window) makes every index the range test admits need one reflection only; the clamp is there so that no read relies on
// that argument.
VP_FLOW_HD static inline int vp_lk_reflect(int i, int n)
{
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// NULL: admitted; else the reason (VP_ERR_INVALID).  What does not depend on pointers.
static inline const char* vp_lk_refusal(int w, int h, int win_w, int win_h, int n, int max_level, int max_count, double eps, int flags, double min_eig_threshold)
{
    (void)max_count;
    if (w < 1 || h < 1 || w > LK_MAX_SIDE || h > LK_MAX_SIDE) return "optical flow: width and height must be 1 to 4096";
    if (win_w < LK_MIN_WIN || win_h < LK_MIN_WIN || win_w > LK_MAX_WIN || win_h > LK_MAX_WIN) return "optical flow: a window side must be 3 to 63";
    if (w <= win_w || h <= win_h) return "optical flow: the image must be larger than the window";
    if (n < 1 || n > LK_MAX_POINTS) return "optical flow: 1 to 1048576 points";
    if (max_level < 0 || max_level >= LK_MAX_LEVELS) return "optical flow: maxLevel must be 0 to 15";
    if (flags & ~(LK_USE_INITIAL_FLOW | LK_GET_MIN_EIGENVALS)) return "optical flow: unknown flag bits";
    if (!isfinite(min_eig_threshold)) return "optical flow: minEigThreshold must be finite";
    if (!isfinite(eps)) return "optical flow: epsilon must be finite";
    return nullptr;
}

static inline int vp_lk_max_count(int max_count) { return max_count < 0 ? 0 : (max_count > LK_MAX_COUNT ? LK_MAX_COUNT : max_count); }
static inline double vp_lk_eps2(double eps)
{
    const double e = eps < 0 ? 0 : (eps > LK_MAX_EPS ? LK_MAX_EPS : eps);
    return e * e;
}

// arguments as vp_lk_refusal admitted them
static inline void vp_lk_make_plan(int w, int h, int win_w, int win_h, int n, int max_level, vp_lk_plan* P)
{
    P->levels = vp_lk_level_count(w, h, win_w, win_h, max_level);
    for (int l = 0; l < LK_MAX_LEVELS; l++) {
        P->cols[l] = l < P->levels ? w : 0;
        P->rows[l] = l < P->levels ? h : 0;
        w = vp_lk_half(w);
        h = vp_lk_half(h);
    }
    P->patch_w = win_w + 3;
    P->patch_h = win_h + 3;
    P->off_deriv = ((size_t)P->patch_w * P->patch_h + 3) / 4 * 4;
    P->off_win = P->off_deriv + (size_t)(win_w + 1) * (win_h + 1) * 4;
    P->lds_bytes = (P->off_win + (size_t)win_w * win_h * 6 + 3) / 4 * 4;
    P->grid = (unsigned)n;
}

static_assert(((size_t)(LK_MAX_WIN + 3) * (LK_MAX_WIN + 3) + 3) / 4 * 4 + (size_t)(LK_MAX_WIN + 1) * (LK_MAX_WIN + 1) * 4 + (size_t)LK_MAX_WIN * LK_MAX_WIN * 6 + 4
                  <= 65536, "optical flow: a point's LDS at 63 x 63 is below the 64 KiB a kernel gets without asking, far below LK_LDS_BYTES");
// exact sums: |Ix|, |Iy| <= 16 * 255 and |diff| <= 32 * 255 after the descale, 63 * 63 terms
static_assert((long long)(16 * 255) * (16 * 255) * LK_MAX_WIN * LK_MAX_WIN < (1ll << 53), "optical flow: a structure sum above 2^53");
static_assert((long long)(32 * 255) * (16 * 255) * LK_MAX_WIN * LK_MAX_WIN < (1ll << 53), "optical flow: a mismatch sum above 2^53");
// a bilinear sample before its descale: 2^14 times at most 16 * 255 (a derivative) or 255 (a pixel)
static_assert((long long)(16 * 255) * (1 << LK_W_BITS) + (1 << (LK_W_BITS - 1)) < (1ll << 31), "optical flow: a weighted sample above int32");
