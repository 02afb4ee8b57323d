// Host arithmetic of semi-global stereo matching (vp_sgm.hip): the argument checks, the candidate rectangle (the block matcher's, at this
// block size), the geometry of the three kernel groups, the workspace and its cap, and the enumeration of a direction's lines that the
// kernel and the host routine share.  Plain C++ - no HIP types, no kernels - and a pure function of its arguments, like vp_stereo_plan.h.
// DESIGN.md section 4.36; tests/sgm_restate.py is the statement.
#pragma once
#include "vp_stereo_plan.h"

#define SG_MIN_BLOCK 1
#define SG_MAX_BLOCK 9
#define SG_MAX_DIFF 255          // disp12_max_diff; -1: no left-right check
#define SG_MAX_SUM 65535         // the summed path costs are 16-bit: paths * (2 cap block^2 + p2) must not pass it
#define SG_COST_THREADS 256
#define SG_STRIP 32              // candidate columns of a cost block (one row of them)
#define SG_WAVE 64
#define SG_AGG_THREADS 64        // an aggregation block is one wave
#define SG_SEL_THREADS 256
#define SG_MAX_WS_BYTES ((size_t)4294967296ull)   // 4 GiB: a call whose workspace would be larger is refused

static_assert(SG_MAX_BLOCK * SG_MAX_BLOCK * 2 * SB_MAX_CAP < 65536, "sgm: a window sum above 16 bits");

struct vp_sgm_plan {
    int r;
    int cx0, cy0, cw, ch;          // the candidate rectangle (cw or ch 0: nothing but the fill is launched)
    // cost: a block makes one candidate row of SG_STRIP columns; two disparities to a 32-bit word, as in the block matcher
    int ndp, ncols, nrcols, lpitch, rpitch;
    int off_v, off_rows;           // LDS offsets in 32-bit words
    unsigned cost_gx, cost_gy;
    size_t cost_lds;
    // aggregation and selection: `group` lanes hold a pixel's disparities, `per_lane` consecutive ones each (lane l of the group holds
    // d = l per_lane ... l per_lane + per_lane - 1; slots at d >= n are idle); a wave holds SG_WAVE / group lines or pixels
    int group, per_lane, lines_per_block;
    unsigned agg_gh, agg_gv, agg_gd;   // blocks of a horizontal, a vertical and a diagonal direction (agg_gd 0 with four paths)
    int px_per_block;
    unsigned sel_g;
    size_t pitch;                  // bytes of a prefiltered row
    size_t off_right, off_c, off_s, ws_bytes;   // the prefiltered left image is at 0; C and S are uint16 [ch][cw][n]
};

// The directions of travel (dy, dx) in the order they are summed: the first four with paths = 4, all with 8
static const int vp_sgm_dirs[8][2] = {{0, 1}, {0, -1}, {1, 0}, {-1, 0}, {1, 1}, {1, -1}, {-1, 1}, {-1, -1}};

VP_STEREO_HD static inline int vp_sgm_line_count(int cw, int ch, int dy, int dx) { return dy == 0 ? ch : (dx == 0 ? cw : cw + ch - 1); }

// line l of direction (dy, dx) over a cw x ch rectangle: its first pixel (the one whose predecessor lies outside) and its length
VP_STEREO_HD static inline void vp_sgm_line(int cw, int ch, int dy, int dx, int l, int* x, int* y, int* len)
{
    const int xs = dx > 0 ? 0 : cw - 1, ys = dy > 0 ? 0 : ch - 1;
    if (dy == 0) { *x = xs; *y = l; *len = cw; return; }
    if (dx == 0) { *x = l; *y = ys; *len = ch; return; }
    // a diagonal starts on the edge row (l < cw) or further down the edge column
    const int x0 = l < cw ? l : xs, y0 = l < cw ? ys : ys + dy * (l - cw + 1);
    const int nx = dx > 0 ? cw - x0 : x0 + 1, ny = dy > 0 ? ch - y0 : y0 + 1;
    *x = x0;
    *y = y0;
    *len = nx < ny ? nx : ny;
}

static inline size_t vp_sgm_workspace(int w, int h, int nd, int cw, int ch, size_t* pitch, size_t* off_right, size_t* off_c, size_t* off_s)
{
    const size_t p = (size_t)(w + 3) / 4 * 4, img = vp_stereo_align(p * h), vol = vp_stereo_align((size_t)cw * ch * nd * 2);
    if (pitch) *pitch = p;
    if (off_right) *off_right = img;
    if (off_c) *off_c = 2 * img;
    if (off_s) *off_s = 2 * img + vol;
    return 2 * img + 2 * vol;
}

static inline void vp_sgm_rect(int w, int h, int nd, int block, int min_disp, int* cx0, int* cy0, int* cw, int* ch)
{
    const int r = block / 2, dmax = min_disp + nd - 1;
    *cx0 = r + (dmax > 0 ? dmax : 0);
    const int cx1 = w - 1 - r + (min_disp < 0 ? min_disp : 0);
    *cy0 = r;
    *cw = cx1 >= *cx0 ? cx1 - *cx0 + 1 : 0;
    *ch = h - 1 - r >= r ? h - 2 * r : 0;
    if (!*cw || !*ch) *cw = *ch = 0;
}

// NULL: admitted; else the reason (VP_ERR_INVALID).  The six arguments a plan depends on.
static inline const char* vp_sgm_geometry_refusal(int w, int h, int nd, int block, int min_disp, int paths)
{
    if (w < 1 || h < 1) return "sgm: width and height must be at least 1";
    if (w > SB_MAX_SIDE || h > SB_MAX_SIDE) return "sgm: width and height must be at most 4096";
    if (nd < SB_MIN_ND || nd > SB_MAX_ND || nd % 16) return "sgm: num_disparities must be a multiple of 16 in 16..256";
    if (block < SG_MIN_BLOCK || block > SG_MAX_BLOCK || block % 2 == 0) return "sgm: block_size must be odd, 1..9";
    if (min_disp < -SB_MAX_MIN_DISP || min_disp > SB_MAX_MIN_DISP) return "sgm: min_disparity must lie in -128..128";
    if (paths != 4 && paths != 8) return "sgm: paths must be 4 or 8";
    int cx0, cy0, cw, ch;
    vp_sgm_rect(w, h, nd, block, min_disp, &cx0, &cy0, &cw, &ch);
    if (vp_sgm_workspace(w, h, nd, cw, ch, nullptr, nullptr, nullptr, nullptr) > SG_MAX_WS_BYTES) return "sgm: the workspace of this call would exceed 4 GiB (4294967296 bytes)";
    return nullptr;
}

// strides in bytes; disp_stride of the int16 result
static inline const char* vp_sgm_refusal(int w, int h, size_t lstride, size_t rstride, int nd, int block, int min_disp, int cap, int p1, int p2, int uniq, int diff, int paths,
                                         size_t disp_stride)
{
    if (const char* why = vp_sgm_geometry_refusal(w, h, nd, block, min_disp, paths)) return why;
    if (cap < 1 || cap > SB_MAX_CAP) return "sgm: pre_filter_cap must lie in 1..63";
    if (p1 < 0 || p2 < 0) return "sgm: p1 and p2 must not be negative";
    if (p1 > p2) return "sgm: p1 must not exceed p2";
    if (uniq < 0 || uniq > 100) return "sgm: uniqueness_ratio must lie in 0..100";
    if (diff < -1 || diff > SG_MAX_DIFF) return "sgm: disp12_max_diff must lie in -1..255";
    if ((long long)paths * (2ll * cap * block * block + p2) > SG_MAX_SUM) return "sgm: paths * (2 * pre_filter_cap * block_size^2 + p2) must not exceed 65535";
    if (lstride < (size_t)w || rstride < (size_t)w) return "sgm: an image's stride is below the row";
    if (disp_stride < (size_t)w * 2) return "sgm: the result's stride is below the row";
    if (disp_stride % 2) return "sgm: the result's stride is not a multiple of the element size";
    return nullptr;
}

// arguments as vp_sgm_geometry_refusal admitted them
static inline void vp_sgm_make_plan(int w, int h, int nd, int block, int min_disp, int paths, vp_sgm_plan* P)
{
    const int r = block / 2;
    P->r = r;
    vp_sgm_rect(w, h, nd, block, min_disp, &P->cx0, &P->cy0, &P->cw, &P->ch);
    P->ndp = nd / 2;
    P->ncols = SG_STRIP + 2 * r;
    P->nrcols = P->ncols + nd - 1;
    P->lpitch = (P->ncols + 3) / 4 * 4;
    P->rpitch = (P->nrcols + 3) / 4 * 4;
    P->off_v = 0;
    P->off_rows = P->ncols * P->ndp;
    P->cost_lds = (size_t)P->off_rows * 4 + (size_t)block * (P->lpitch + P->rpitch);
    P->cost_gx = (unsigned)((P->cw + SG_STRIP - 1) / SG_STRIP);
    P->cost_gy = (unsigned)P->ch;
    P->per_lane = nd <= 64 ? 1 : (nd <= 128 ? 2 : 4);
    P->group = nd <= 16 ? 16 : (nd <= 32 ? 32 : 64);
    P->lines_per_block = SG_WAVE / P->group;
    const int lpb = P->lines_per_block;
    P->agg_gh = (unsigned)((P->ch + lpb - 1) / lpb);
    P->agg_gv = (unsigned)((P->cw + lpb - 1) / lpb);
    P->agg_gd = paths == 8 && P->cw ? (unsigned)((P->cw + P->ch - 1 + lpb - 1) / lpb) : 0u;
    P->px_per_block = SG_SEL_THREADS / P->group;
    P->sel_g = (unsigned)(((size_t)P->cw * P->ch + P->px_per_block - 1) / P->px_per_block);
    P->ws_bytes = vp_sgm_workspace(w, h, nd, P->cw, P->ch, &P->pitch, &P->off_right, &P->off_c, &P->off_s);
}

static_assert(((SG_STRIP + SG_MAX_BLOCK - 1) * (SB_MAX_ND / 2)) * 4 + SG_MAX_BLOCK * (2 * (SG_STRIP + SG_MAX_BLOCK + 2) + SB_MAX_ND) <= SB_LDS_BYTES,
              "sgm: the cost block's tables above the LDS budget");
