// Host arithmetic of the derivative filters (vpk_deriv, vp_deriv.hip): the argument check of cv2.Sobel / Scharr / Laplacian /
// spatialGradient, the integer taps of cv::getDerivKernels, which kernel instantiation serves a call, and the launch geometry; and
// the border index map, which the kernels share with the host.  Plain C++ - no HIP types, no kernels - and a pure function of its
// arguments, like vp_median_plan.h.  The codes are those of include/vp.h (vp_deriv.hip asserts that they agree).
#pragma once

#ifdef __HIPCC__
#define VP_DERIV_HD __host__ __device__
#else
#define VP_DERIV_HD
#endif

// the tile of every kernel (the kernels assert their LDS budgets from the same numbers)
#define DV_EPL 8               // adjacent results per lane: one 8-byte store of uint8, one 16-byte store of int16, two / four of float / double
#define DV_TB 512              // results (bytes of a source row) per tile row: 64 lanes x DV_EPL, one wave per result row
#define DV_TH 16               // result rows per tile
#define DV_MAXK 7              // largest tap count
#define DV_PAD 12              // staged bytes in front of the tile's first result byte: >= (DV_MAXK / 2) * 4 channels, whole dwords

enum { VP_DV_OP_SOBEL = 0, VP_DV_OP_SCHARR = 1, VP_DV_OP_LAPLACIAN = 2, VP_DV_OP_SPATIAL_GRADIENT = 3 };
enum { VP_DV_8U = 0, VP_DV_16S = 3, VP_DV_32F = 5, VP_DV_64F = 6 };                                  // cv2's depth codes
enum { VP_DV_CONSTANT = 0, VP_DV_REPLICATE = 1, VP_DV_REFLECT = 2, VP_DV_REFLECT_101 = 4, VP_DV_ISOLATED = 16 };   // cv2's border codes
// kernels: one separable term; the sum of two (Laplacian 5, 7); two terms to two planes (spatialGradient); a 3x3 Laplacian run directly
enum { VP_DV_KERNEL_ONE = 0, VP_DV_KERNEL_SUM = 1, VP_DV_KERNEL_PAIR = 2, VP_DV_KERNEL_LAP3 = 3 };

// cv::borderInterpolate: the index inside [0, len) that coordinate p of the extended image reads, -1 for the constant border (value 0)
VP_DERIV_HD static inline int vp_deriv_border_index(int p, int len, int border)
{
    if ((unsigned)p < (unsigned)len) return p;
    if (border == VP_DV_REPLICATE) return p < 0 ? 0 : len - 1;
    if (border == VP_DV_CONSTANT) return -1;
    if (len == 1) return 0;
    const int delta = border == VP_DV_REFLECT_101 ? 1 : 0;
    do {
        p = p < 0 ? -p - 1 + delta : len - 1 - (p - len) - delta;
    } while ((unsigned)p >= (unsigned)len);
    return p;
}

// Taps of one term: plane = the row filter `row` over the extended source row, result = the column filter `col` over the plane.
// Term B is used by VP_DV_KERNEL_SUM (added to term A) and VP_DV_KERNEL_PAIR (the second output).  Entries [0, K).
struct vp_deriv_taps { int rowA[DV_MAXK], colA[DV_MAXK], rowB[DV_MAXK], colB[DV_MAXK]; };

struct vp_deriv_plan {
    int ok;                    // 0: the arguments are outside what cv2 and this library accept
    int kernel;                // VP_DV_KERNEL_*
    int K;                     // taps per axis: 3, 5 or 7
    int depth;                 // VP_DV_8U / 16S / 32F / 64F (-1 resolved)
    int esize;                 // bytes per result element
    int border;                // VP_DV_CONSTANT / REPLICATE / REFLECT / REFLECT_101 (the ISOLATED bit dropped)
    vp_deriv_taps taps;
    int lap_corner, lap_edge, lap_centre;   // VP_DV_KERNEL_LAP3: the 3x3 kernel's three distinct weights
    unsigned gx, gy, block;    // launch geometry
};

// cv::getSobelKernels for one axis: n taps of derivative order `order` (n > order): n - 1 - order convolutions of [1 1], then `order`
// of [-1 1].  n = 3: [1 2 1], [-1 0 1], [1 -2 1].
static inline void vp_deriv_sobel_taps(int n, int order, int* t)
{
    for (int i = 0; i < DV_MAXK; i++) t[i] = 0;
    t[0] = 1;
    for (int len = 1; len < n; len++) {
        const int a = len > n - 1 - order ? -1 : 1;             // the next factor is [a 1]
        for (int i = len; i >= 0; i--) t[i] = (i > 0 ? t[i - 1] : 0) + a * (i < len ? t[i] : 0);
    }
}

// op: VP_DV_OP_*; ksize as cv2 takes it (Sobel: 1, 3, 5, 7 or -1 = Scharr; Laplacian: 1, 3, 5, 7; spatialGradient: 3); ddepth: -1 or a
// VP_DV_* depth; border: a VP_DV_* border code, the ISOLATED bit ignored.
static inline vp_deriv_plan vp_deriv_make_plan(int w, int h, int cn, int op, int dx, int dy, int ksize, int ddepth, int border)
{
    vp_deriv_plan P;
    P.ok = 0;
    P.kernel = VP_DV_KERNEL_ONE;
    P.K = 3;
    P.depth = ddepth < 0 ? VP_DV_8U : ddepth;
    P.esize = P.depth == VP_DV_8U ? 1 : P.depth == VP_DV_16S ? 2 : P.depth == VP_DV_32F ? 4 : 8;
    P.border = border & ~VP_DV_ISOLATED;
    P.lap_corner = P.lap_edge = P.lap_centre = 0;
    P.gx = P.gy = P.block = 0;
    for (int i = 0; i < DV_MAXK; i++) P.taps.rowA[i] = P.taps.colA[i] = P.taps.rowB[i] = P.taps.colB[i] = 0;
    if (w <= 0 || h <= 0 || h > 65535 || cn < 1 || cn > 4 || (long long)w * cn > (1ll << 30)) return P;
    if (ddepth != -1 && ddepth != VP_DV_8U && ddepth != VP_DV_16S && ddepth != VP_DV_32F && ddepth != VP_DV_64F) return P;
    if (P.border != VP_DV_CONSTANT && P.border != VP_DV_REPLICATE && P.border != VP_DV_REFLECT && P.border != VP_DV_REFLECT_101) return P;
    if (op == VP_DV_OP_SOBEL && ksize == -1) op = VP_DV_OP_SCHARR;
    if (op == VP_DV_OP_SOBEL) {
        if (dx < 0 || dy < 0 || dx > 2 || dy > 2 || dx + dy <= 0) return P;
        if (ksize != 1 && ksize != 3 && ksize != 5 && ksize != 7) return P;
        if (ksize > 1 && (dx >= ksize || dy >= ksize)) return P;
        P.K = ksize == 1 ? 3 : ksize;
        vp_deriv_sobel_taps(P.K, dx, P.taps.rowA);
        vp_deriv_sobel_taps(P.K, dy, P.taps.colA);
        if (ksize == 1) {                                       // an axis that is not differentiated keeps its single tap [1]
            if (dx == 0) { P.taps.rowA[0] = 0; P.taps.rowA[1] = 1; P.taps.rowA[2] = 0; }
            if (dy == 0) { P.taps.colA[0] = 0; P.taps.colA[1] = 1; P.taps.colA[2] = 0; }
        }
    } else if (op == VP_DV_OP_SCHARR) {
        if (dx < 0 || dy < 0 || dx + dy != 1) return P;
        int* d = dx ? P.taps.rowA : P.taps.colA;
        int* s = dx ? P.taps.colA : P.taps.rowA;
        d[0] = -1; d[1] = 0; d[2] = 1;
        s[0] = 3; s[1] = 10; s[2] = 3;
    } else if (op == VP_DV_OP_LAPLACIAN) {
        if (ksize == 1 || ksize == 3) {
            P.kernel = VP_DV_KERNEL_LAP3;
            P.lap_corner = ksize == 1 ? 0 : 2;
            P.lap_edge = ksize == 1 ? 1 : 0;
            P.lap_centre = ksize == 1 ? -4 : -8;
        } else if (ksize == 5 || ksize == 7) {                  // Sobel(2, 0, ksize) + Sobel(0, 2, ksize)
            P.kernel = VP_DV_KERNEL_SUM;
            P.K = ksize;
            vp_deriv_sobel_taps(ksize, 2, P.taps.rowA);
            vp_deriv_sobel_taps(ksize, 0, P.taps.colA);
            vp_deriv_sobel_taps(ksize, 0, P.taps.rowB);
            vp_deriv_sobel_taps(ksize, 2, P.taps.colB);
        } else {
            return P;
        }
    } else if (op == VP_DV_OP_SPATIAL_GRADIENT) {               // (dx, dy) = Sobel(1, 0, 3), Sobel(0, 1, 3), both int16
        if (ksize != 3 || cn != 1 || (P.border != VP_DV_REFLECT_101 && P.border != VP_DV_REPLICATE)) return P;
        P.kernel = VP_DV_KERNEL_PAIR;
        P.depth = VP_DV_16S;
        P.esize = 2;
        vp_deriv_sobel_taps(3, 1, P.taps.rowA);
        vp_deriv_sobel_taps(3, 0, P.taps.colA);
        vp_deriv_sobel_taps(3, 0, P.taps.rowB);
        vp_deriv_sobel_taps(3, 1, P.taps.colB);
    } else {
        return P;
    }
    P.gx = (unsigned)(((long long)w * cn + DV_TB - 1) / DV_TB);
    P.gy = (unsigned)((h + DV_TH - 1) / DV_TH);
    P.block = 256;
    P.ok = 1;
    return P;
}
