// Host arithmetic of stereo block matching (vp_stereo.hip): the argument checks, the candidate rectangle, the strip and band geometry of
// the matcher with its LDS layout, the workspace, and the two formulas the kernel and the host routine share (subpixel result, depth).
// Plain C++ - no HIP types, no kernels - and a pure function of its arguments, like vp_match_plan.h.  DESIGN.md section 4.34;
// tests/stereo_restate.py is the statement.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define SB_MAX_SIDE 4096
#define SB_MIN_ND 16
#define SB_MAX_ND 256
#define SB_MIN_BLOCK 5
#define SB_MAX_BLOCK 21
#define SB_MAX_MIN_DISP 128      // |min_disparity|
#define SB_MAX_CAP 63
#define SB_THREADS 256
#define SB_STRIP_WIDE 64         // candidate columns of a strip, num_disparities <= SB_WIDE_MAX_ND
#define SB_STRIP_NARROW 32       // ... above it: the two LDS tables grow with strip x disparities
#define SB_WIDE_MAX_ND 128
#define SB_MIN_BAND_ROWS 16      // a band pays 2 r rows of column sums before its first result row
#define SB_WANT_BLOCKS 512       // bands are cut until the grid has about two blocks per compute unit
#define SB_LDS_BYTES 65536       // dynamic LDS a block of this library may use

// every window sum fits 16 bits, which is what lets two disparities share a 32-bit LDS word
static_assert(SB_MAX_BLOCK * SB_MAX_BLOCK * 2 * SB_MAX_CAP < 65536, "stereo: a window sum above 16 bits");
static_assert(SB_THREADS % SB_STRIP_WIDE == 0 && SB_THREADS % SB_STRIP_NARROW == 0, "stereo: the scan splits the disparities among threads / strip lanes per pixel");
static_assert(SB_MIN_ND % (SB_THREADS / SB_STRIP_NARROW) == 0, "stereo: every scan part holds a whole number of disparities");

#ifdef __HIPCC__
#define VP_STEREO_HD __host__ __device__
#else
#define VP_STEREO_HD
#endif

struct vp_stereo_plan {
    int r;                         // block_size / 2
    int cx0, cy0, cw, ch;          // the candidate rectangle (cw or ch 0: no candidate pixel, nothing but the fill is launched)
    int strip_cols, band_rows;     // a block owns strip_cols candidate columns of band_rows candidate rows
    unsigned grid_x, grid_y;
    int ndp;                       // disparity pairs, num_disparities / 2: two 16-bit sums per LDS word
    int ncols;                     // columns of vertical sums a strip keeps, strip_cols + 2 r
    int nrcols;                    // columns of the right image under them, ncols + num_disparities - 1
    int parts;                     // threads that share a pixel's scan over the disparities, SB_THREADS / strip_cols
    int segs, seg_cols;            // the horizontal pass: segs column segments of seg_cols per disparity pair
    int hpitch;                    // 16-bit entries of a row of the window-sum table, strip_cols + 2 (an odd number of words)
    // LDS, offsets in 32-bit words
    int off_v, off_h, off_t, off_rows, off_red;
    int lpitch, rpitch;            // bytes of a staged left / right row (multiples of 4)
    size_t lds_bytes;
    size_t pitch;                  // bytes of a prefiltered row in the workspace
    size_t off_right, ws_bytes;    // the prefiltered left image is at 0
};

// NULL: admitted; else the reason (VP_ERR_INVALID).  The five arguments a plan depends on.
static inline const char* vp_stereo_geometry_refusal(int w, int h, int nd, int block, int min_disp)
{
    if (w < 1 || h < 1) return "stereo: width and height must be at least 1";
    if (w > SB_MAX_SIDE || h > SB_MAX_SIDE) return "stereo: width and height must be at most 4096";
    if (nd < SB_MIN_ND || nd > SB_MAX_ND || nd % 16) return "stereo: num_disparities must be a multiple of 16 in 16..256";
    if (block < SB_MIN_BLOCK || block > SB_MAX_BLOCK || block % 2 == 0) return "stereo: block_size must be odd, 5..21";
    if (min_disp < -SB_MAX_MIN_DISP || min_disp > SB_MAX_MIN_DISP) return "stereo: min_disparity must lie in -128..128";
    return nullptr;
}

// strides in bytes; disp_stride of the int16 result
static inline const char* vp_stereo_bm_refusal(int w, int h, size_t lstride, size_t rstride, int nd, int block, int min_disp, int cap, int texture, int uniq,
                                               size_t disp_stride)
{
    if (const char* why = vp_stereo_geometry_refusal(w, h, nd, block, min_disp)) return why;
    if (cap < 1 || cap > SB_MAX_CAP) return "stereo: pre_filter_cap must lie in 1..63";
    if (texture < 0) return "stereo: texture_threshold must not be negative";
    if (uniq < 0 || uniq > 100) return "stereo: uniqueness_ratio must lie in 0..100";
    if (lstride < (size_t)w || rstride < (size_t)w) return "stereo: an image's stride is below the row";
    if (disp_stride < (size_t)w * 2) return "stereo: the result's stride is below the row";
    if (disp_stride % 2) return "stereo: the result's stride is not a multiple of the element size";
    return nullptr;
}

static inline const char* vp_depth_refusal(int w, int h, size_t disp_stride, size_t depth_stride)
{
    if (w < 1 || h < 1) return "depth: width and height must be at least 1";
    if (w > SB_MAX_SIDE || h > SB_MAX_SIDE) return "depth: width and height must be at most 4096";
    if (disp_stride < (size_t)w * 2) return "depth: the disparity's stride is below the row";
    if (disp_stride % 2) return "depth: the disparity's stride is not a multiple of the element size";
    if (depth_stride < (size_t)w * 4) return "depth: the result's stride is below the row";
    if (depth_stride % 4) return "depth: the result's stride is not a multiple of the element size";
    return nullptr;
}

VP_STEREO_HD static inline int vp_stereo_invalid(int min_disp) { return (min_disp - 1) * 16; }

// the int16 result of a pixel that passed the texture and uniqueness tests: cmin = C(D*), pm = C(D* - 1), pp = C(D* + 1) (mirrored at an
// end of the range by the caller), D the disparity itself
VP_STEREO_HD static inline int16_t vp_stereo_subpixel(int cmin, int pm, int pp, int D)
{
    const int diff = pm - pp, den = pm + pp - 2 * cmin + (diff < 0 ? -diff : diff);
    const int off = den ? diff * 256 / den : 0;
    return (int16_t)((D * 256 + off + 15) >> 4);
}

// fb: focal_px * baseline_m as one double product, made on the host
VP_STEREO_HD static inline float vp_stereo_depth(double fb, int disp16) { return disp16 > 0 ? (float)(fb * 16.0 / (double)disp16) : 0.0f; }

// XSOBEL of one host image into rows of w bytes: what the host routines of the block matcher and of semi-global matching start from
static inline void vp_stereo_host_prefilter(const uint8_t* src, size_t stride, int w, int h, int cap, uint8_t* out)
{
    for (int y = 0; y < h; y++) {
        const int ya = h == 1 ? 0 : (y == 0 ? 1 : y - 1), yb = h == 1 ? 0 : (y == h - 1 ? h - 2 : y + 1);
        const uint8_t *a = src + (size_t)ya * stride, *m = src + (size_t)y * stride, *b = src + (size_t)yb * stride;
        uint8_t* o = out + (size_t)y * w;
        for (int x = 0; x < w; x++) {
            int v = 0;
            if (x >= 1 && x <= w - 2) {
                v = (int)a[x + 1] - (int)a[x - 1] + 2 * ((int)m[x + 1] - (int)m[x - 1]) + (int)b[x + 1] - (int)b[x - 1];
                v = v < -cap ? -cap : (v > cap ? cap : v);
            }
            o[x] = (uint8_t)(v + cap);
        }
    }
}

static inline size_t vp_stereo_align(size_t n) { return (n + 255) / 256 * 256; }

// arguments as vp_stereo_geometry_refusal admitted them
static inline void vp_stereo_make_plan(int w, int h, int nd, int block, int min_disp, vp_stereo_plan* P)
{
    const int r = block / 2, dmax = min_disp + nd - 1;
    P->r = r;
    // r <= x <= w - 1 - r, x - r - dmax >= 0, x + r - min_disp <= w - 1
    P->cx0 = r + (dmax > 0 ? dmax : 0);
    const int cx1 = w - 1 - r + (min_disp < 0 ? min_disp : 0);
    P->cy0 = r;
    P->cw = cx1 >= P->cx0 ? cx1 - P->cx0 + 1 : 0;
    P->ch = h - 1 - r >= r ? h - 2 * r : 0;
    if (!P->cw || !P->ch) P->cw = P->ch = 0;
    P->strip_cols = nd <= SB_WIDE_MAX_ND ? SB_STRIP_WIDE : SB_STRIP_NARROW;
    P->grid_x = (unsigned)((P->cw + P->strip_cols - 1) / P->strip_cols);
    const int want = P->grid_x ? (int)((SB_WANT_BLOCKS + P->grid_x - 1) / P->grid_x) : 1;
    P->band_rows = (P->ch + want - 1) / want;
    if (P->band_rows < SB_MIN_BAND_ROWS) P->band_rows = SB_MIN_BAND_ROWS;
    P->grid_y = (unsigned)((P->ch + P->band_rows - 1) / P->band_rows);
    P->ndp = nd / 2;
    P->ncols = P->strip_cols + 2 * r;
    P->nrcols = P->ncols + nd - 1;
    P->parts = SB_THREADS / P->strip_cols;
    P->segs = SB_THREADS / P->ndp;
    if (P->segs > P->strip_cols) P->segs = P->strip_cols;
    P->seg_cols = (P->strip_cols + P->segs - 1) / P->segs;
    P->hpitch = P->strip_cols + 2;
    P->lpitch = (P->ncols + 3) / 4 * 4;
    P->rpitch = (P->nrcols + 3) / 4 * 4;
    P->off_v = 0;
    P->off_h = P->off_v + P->ncols * P->ndp;
    P->off_t = P->off_h + nd * (P->hpitch / 2);
    P->off_rows = P->off_t + P->ncols;
    P->off_red = P->off_rows + (2 * P->lpitch + 2 * P->rpitch) / 4;
    P->lds_bytes = (size_t)(P->off_red + 2 * SB_THREADS) * 4;
    P->pitch = (size_t)(w + 3) / 4 * 4;
    P->off_right = vp_stereo_align(P->pitch * h);
    P->ws_bytes = 2 * P->off_right;
}

// the largest block of either strip width stays inside the budget: (ncols ndp + nd hpitch / 2 + ncols + rows + scan) words
static_assert(((SB_STRIP_WIDE + SB_MAX_BLOCK - 1) * (SB_WIDE_MAX_ND / 2) + SB_WIDE_MAX_ND * (SB_STRIP_WIDE + 2) / 2 + (SB_STRIP_WIDE + SB_MAX_BLOCK - 1) +
               (SB_STRIP_WIDE + SB_MAX_BLOCK + 2) + (SB_STRIP_WIDE + SB_MAX_BLOCK + SB_WIDE_MAX_ND + 2) / 2 + 2 * SB_THREADS) * 4 <= SB_LDS_BYTES,
              "stereo: the wide strip's tables above the LDS budget");
static_assert(((SB_STRIP_NARROW + SB_MAX_BLOCK - 1) * (SB_MAX_ND / 2) + SB_MAX_ND * (SB_STRIP_NARROW + 2) / 2 + (SB_STRIP_NARROW + SB_MAX_BLOCK - 1) +
               (SB_STRIP_NARROW + SB_MAX_BLOCK + 2) + (SB_STRIP_NARROW + SB_MAX_BLOCK + SB_MAX_ND + 2) / 2 + 2 * SB_THREADS) * 4 <= SB_LDS_BYTES,
              "stereo: the narrow strip's tables above the LDS budget");
