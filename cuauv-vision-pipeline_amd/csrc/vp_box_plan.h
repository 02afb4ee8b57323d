// Host arithmetic of the box filter, the two pyramid steps and the integral image (vp_box.hip, vp_pyr.hip, vp_integral.hip): the
// argument checks of cv2.boxFilter / blur / pyrDown / pyrUp / integral, which kernels serve a box call (one LDS-tiled pass or two
// passes with a uint16 image of row sums between them), the launch geometry, and the admission of a normalised window's area.
// Plain C++ - no HIP types, no kernels - and a pure function of its arguments, like vp_deriv_plan.h, whose border index map and
// border / depth codes it shares.  tests/box_pyr_restate.py is the statement the kernels are held to.
#pragma once
#include <math.h>
#include "vp_deriv_plan.h"

// ---- box filter ---------------------------------------------------------------------------------------------------------------------
#define BX_TB 256              // result bytes per tile row: one thread per result column
#define BX_TH 32               // result rows per tile of the one-pass kernel
#define BX_CHUNK 12            // staged bytes one lane scans in the one-pass kernel: a multiple of every channel count 1..4
#define BX_ROW_CHUNK 24        // the same in the row kernel of the two-pass path
#define BX_LDS_BYTES 61440     // dynamic LDS the one-pass kernel may ask for
#define BX_STRIP 64            // least result rows per block of the column kernel of the two-pass path
#define BX_MAXK 255            // largest window side: a row sum (<= 255 * 255) fits uint16, a window sum int32
// ---- pyramid steps (tiles in pixels) ------------------------------------------------------------------------------------------------
#define PD_TW 64               // pyrDown: result pixels per tile row; the staged source tile is (2 PD_TH + 4) x (2 PD_TW + 4) pixels
#define PD_TH 16               // pyrDown: result rows per tile
#define PU_TW 64               // pyrUp: source pixels per tile row; staged (PU_TH + 2) x (PU_TW + 2), result 2 PU_TH x 2 PU_TW
#define PU_TH 8                // pyrUp: source rows per tile
// ---- integral -----------------------------------------------------------------------------------------------------------------------
#define IG_CHUNK 12            // source bytes per lane and scan step
#define IG_SCAN 768            // one scan block: the bytes of a row one wave scans per step (64 lanes x IG_CHUNK), carried into the next
#define IG_COLS 64             // columns per block of the column scan

enum { VP_BX_32S = 4 };                                          // cv2's CV_32S, beside VP_DV_8U / 16S / 32F / 64F
enum { VP_BX_STORE_8U = 0, VP_BX_STORE_8U_NORM = 1, VP_BX_STORE_16S = 2, VP_BX_STORE_32S = 3, VP_BX_STORE_32F = 4, VP_BX_STORE_64F = 5 };

// round-half-to-even of s / area as one integer expression: q = ((2 s + area) * mul) >> shift = floor((2 s + area) / (2 area)), one
// less where that division is exact and q is odd.  mul and shift come from vp_box_make_div.
struct vp_box_div { unsigned area, mul; int shift; };
VP_DERIV_HD static inline unsigned vp_box_mean(unsigned s, const vp_box_div d)
{
    const unsigned n = 2u * s + d.area;
    unsigned q = (unsigned)(((unsigned long long)n * d.mul) >> d.shift);
    if (n == q * 2u * d.area && (q & 1u)) q--;
    return q;
}

static inline vp_box_div vp_box_make_div(int area)           // 1 <= area <= BX_MAXK^2
{
    vp_box_div d;
    d.area = (unsigned)area;
    int L = 1;
    while ((1u << L) < 2u * d.area) L++;
    d.shift = 26 + L;                                            // 2 s + area < 2^26 and 2 area <= 2^L: the product is exact below 2^shift
    d.mul = (unsigned)((1ull << d.shift) / (2u * d.area) + 1);
    return d;
}

// Whether cv2's three roundings of sum / area give one byte for every sum 0 .. 255 * area (so that a normalised window of that area
// can be restated), and vp_box_mean gives the same: 1 / 0, negative for area < 1 or above BX_MAXK^2.  OpenCV scales a 16-bit sum by a
// Q23 reciprocal when area <= 256 (ColumnSum<ushort, uchar>), else an int32 sum by the float32 product in its vector body and by the
// double product in its scalar tail (ColumnSum<int, uchar>), both rounded half to even.  Enumerates: 255 * area steps.
static inline int vp_box_area_admit(int area)
{
    if (area < 1 || area > BX_MAXK * BX_MAXK) return -1;
    if (area == 1) return 1;                                     // scale == 1: OpenCV scales nothing, and vp_box_mean(s) = s
    const vp_box_div d = vp_box_make_div(area);
    const double scale = 1.0 / area;
    const float scalef = (float)scale;
    const double q23 = (double)(1 << 23) / area;
    unsigned div_scale = (unsigned)floor(q23), div_delta = (unsigned)area / 2;
    if (q23 - div_scale < 0.5) div_delta++; else div_scale++;
    const unsigned top = 255u * d.area;
    for (unsigned s = 0; s <= top; s++) {
        const unsigned m = vp_box_mean(s, d);
        const volatile float pf = (float)s * scalef;             // (volatile: the products are rounded to their types before rint)
        const volatile double pd = (double)s * scale;
        if ((unsigned)lrintf(pf) != m || (unsigned)lrint(pd) != m) return 0;
        if (area <= 256 && (unsigned)(((unsigned long long)(s + div_delta) * div_scale) >> 23) != m) return 0;
    }
    return 1;
}

struct vp_box_plan {
    int ok;                    // 0: the arguments are outside what cv2 and this library accept
    int kw, kh, ax, ay;        // window and anchor (kw / 2, kh / 2)
    int depth, esize, store;   // VP_DV_* / VP_BX_32S (-1 resolved), bytes per result element, VP_BX_STORE_*
    int border;
    int onepass;               // 1: k_box; 0: k_box_rows + k_box_cols
    int nchunks, pitch, srows; // one pass: lanes that stage a row, uint16 per staged row (4 zeros in front), staged rows of a full tile
    unsigned lds_bytes;        // one pass: dynamic LDS
    int row_out;               // two passes: row sums one wave produces per step
    int strip;                 // two passes: result rows per block of the column kernel
    unsigned gx, gy, gx2, gy2; // grids: one pass / row kernel; column kernel
    vp_box_div div;            // normalised: vp_box_make_div of an area the caller found admitted
};

// staged bytes of a row in the one-pass kernel, lanes that scan them, and the LDS of a tile
static inline int vp_box_onepass_fits(int cn, int kw, int kh, int* nchunks, int* pitch, unsigned* lds)
{
    const int sw = BX_TB + (kw - 1) * cn, nc = (sw + BX_CHUNK - 1) / BX_CHUNK, p = nc * BX_CHUNK + 4;
    const unsigned bytes = (unsigned)(BX_TH + kh - 1) * p * 2u;
    if (nchunks) *nchunks = nc;
    if (pitch) *pitch = p;
    if (lds) *lds = bytes;
    return nc <= 64 && bytes <= BX_LDS_BYTES;
}

// ddepth: -1 or VP_DV_8U / 16S / VP_BX_32S / 32F / 64F; normalize: only with -1 / 8U.  The area's admission is the caller's second check.
static inline vp_box_plan vp_box_make_plan(int w, int h, int cn, int kw, int kh, int normalize, int ddepth, int border)
{
    vp_box_plan P;
    P.ok = 0;
    P.kw = kw; P.kh = kh; P.ax = kw / 2; P.ay = kh / 2;
    P.depth = ddepth < 0 ? VP_DV_8U : ddepth;
    P.esize = P.depth == VP_DV_8U ? 1 : P.depth == VP_DV_16S ? 2 : P.depth == VP_DV_64F ? 8 : 4;
    P.border = border & ~VP_DV_ISOLATED;
    P.store = 0; P.onepass = 0; P.nchunks = P.pitch = P.srows = 0; P.lds_bytes = 0; P.row_out = 0; P.strip = 0;
    P.gx = P.gy = P.gx2 = P.gy2 = 0;
    P.div.area = 1; P.div.mul = 0; P.div.shift = 0;
    if (w <= 0 || h <= 0 || h > 65535 || cn < 1 || cn > 4 || (long long)w * cn > (1ll << 30)) return P;
    if (kw < 1 || kh < 1 || kw > BX_MAXK || kh > BX_MAXK) return P;
    if (P.border != VP_DV_CONSTANT && P.border != VP_DV_REPLICATE && P.border != VP_DV_REFLECT && P.border != VP_DV_REFLECT_101) return P;
    if (normalize) {
        if (P.depth != VP_DV_8U) return P;
        P.store = VP_BX_STORE_8U_NORM;
    } else {
        switch (P.depth) {
            case VP_DV_8U: P.store = VP_BX_STORE_8U; break;
            case VP_DV_16S: P.store = VP_BX_STORE_16S; break;
            case VP_BX_32S: P.store = VP_BX_STORE_32S; break;
            case VP_DV_32F: if (255ll * kw * kh >= (1ll << 24)) return P; P.store = VP_BX_STORE_32F; break;
            case VP_DV_64F: P.store = VP_BX_STORE_64F; break;
            default: return P;
        }
    }
    const long long rb = (long long)w * cn;
    P.onepass = vp_box_onepass_fits(cn, kw, kh, &P.nchunks, &P.pitch, &P.lds_bytes);
    P.srows = BX_TH + kh - 1;
    if (P.onepass) {
        P.gx = (unsigned)((rb + BX_TB - 1) / BX_TB);
        P.gy = (unsigned)((h + BX_TH - 1) / BX_TH);
    } else {
        P.row_out = 64 * BX_ROW_CHUNK - (kw - 1) * cn;           // >= 1536 - 254 * 4
        P.gx = (unsigned)((rb + P.row_out - 1) / P.row_out);
        P.gy = (unsigned)((h + 3) / 4);
        P.strip = kh > BX_STRIP ? kh : BX_STRIP;                 // the kh - 1 rows a block sums before its first result stay below its results
        P.gx2 = (unsigned)((rb + BX_TB - 1) / BX_TB);
        P.gy2 = (unsigned)((h + P.strip - 1) / P.strip);
    }
    P.ok = 1;
    return P;
}

// ---- pyramid steps: sizes and borders -------------------------------------------------------------------------------------------------
static inline int vp_pyr_sizes_ok(int w, int h, int cn) { return w > 0 && h > 0 && h <= 32767 && cn >= 1 && cn <= 4 && (long long)w * cn <= (1ll << 29); }
static inline int vp_pyr_down_border_ok(int border)
{
    border &= ~VP_DV_ISOLATED;
    return border == VP_DV_REFLECT_101 || border == VP_DV_REPLICATE || border == VP_DV_REFLECT;
}
// pyrUp's neighbour of source index q in [-1, n]: -1 reflects without repeating the edge (1, or 0 when n == 1), n replicates (n - 1)
VP_DERIV_HD static inline int vp_pyr_up_index(int q, int n) { return q < 0 ? (n > 1 ? 1 : 0) : (q >= n ? n - 1 : q); }

// ---- integral: the last entry, 255 * w * h, must fit int32 ---------------------------------------------------------------------------
static inline int vp_integral_sizes_ok(int w, int h, int cn)
{
    return w > 0 && h > 0 && cn >= 1 && cn <= 4 && 255ll * w * h <= 2147483647ll;
}
