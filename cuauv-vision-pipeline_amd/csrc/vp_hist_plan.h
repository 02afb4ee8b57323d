// Host arithmetic of cv2.calcHist, cv2.calcBackProject and cv2.meanShift (vp_hist.hip): the argument checks as this library admits
// them, the 256-entry bin tables of cv2's calcHistLookupTables_8u, the choice between counters / tables in LDS and in device memory,
// the grids, the LDS sizes and the layout of the workspace.  Plain C++ - no HIP types, no kernels - and a pure function of its
// arguments, like vp_match_plan.h.  DESIGN.md section 4.28; tests/hist_restate.py is the statement.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define HS_MAX_SIDE 4096       // rows and columns of an image: at most 2^24 pixels, so a count is exact as uint32 and as float32
#define HS_MAX_CN 4
#define HS_MAX_DIMS 3
#define HS_MAX_SIZE 256        // bins per dimension
#define HS_OUT_BIN 65535       // a byte value that falls into no bin

// A gfx950 compute unit has 160 KiB of LDS and one workgroup may take all of it (163,840 bytes).  Both image kernels keep the three
// bin tables as premultiplied int32 offsets in front (HS_TAB_LDS_BYTES), which leaves 160,768 bytes: 40,192 counters or 160,768 table
// bytes.  The two limits below are the largest values within that budget whose neighbours on both sides are products of three sizes
// of 1..256, so that a test can stand one below, at and one above them.
#define HS_LDS_BYTES 163840
#define HS_TAB_LDS_BYTES 3072
#define HS_HIST_LDS_BINS 40171   // counters a block keeps in LDS: above, every lane adds to device memory
#define HS_BP_LDS_BYTES 160370   // bytes of a folded table a block keeps in LDS: above, every lane gathers from device memory
#define HS_THREADS 1024
#define HS_PX 4                  // neighbouring pixels of a row a lane takes at a time
#define HS_MAX_BLOCKS 512        // grid of the image kernels (they stride over the image) ...
#define HS_MAX_BLOCKS_BIG 256    // ... and when a block's LDS is above a quarter of the compute unit's: one block per compute unit
#define HS_OUT_OFFSET (-(1 << 28))   // premultiplied offset of HS_OUT_BIN: any sum that holds one is negative

#define HS_MS_THREADS 1024       // mean shift: one block per window
#define HS_MS_MAX_WINDOWS 4096
#define HS_MS_MAX_ITER 100000

static_assert(HS_TAB_LDS_BYTES == HS_MAX_DIMS * 256 * 4, "hist: three tables of 256 int32");
static_assert(HS_TAB_LDS_BYTES + HS_HIST_LDS_BINS * 4 <= HS_LDS_BYTES, "hist: counters above the LDS of a compute unit");
static_assert(HS_TAB_LDS_BYTES + (HS_BP_LDS_BYTES + 3) / 4 * 4 <= HS_LDS_BYTES, "hist: table above the LDS of a compute unit");
static_assert((long long)HS_MAX_SIZE * HS_MAX_SIZE * HS_MAX_SIZE < -(long long)HS_OUT_OFFSET, "hist: an offset sum could hide HS_OUT_OFFSET");
static_assert((long long)HS_MAX_SIDE * HS_MAX_SIDE <= (1ll << 24), "hist: a count above 2^24 is not exact in float32");
// mean shift: a lane's sums of one row (at most 16 words of 4 pixels) stay in 32 bits, the totals of a window in 53
static_assert(4095ull * 255 * 4 * 16 + 6 * 255 * 16 < (1ull << 32), "mean shift: a lane's row sum above uint32");
static_assert(4095ull * 255 * HS_MAX_SIDE * HS_MAX_SIDE < (1ull << 53), "mean shift: a first moment above 2^53");

struct vp_hist_tabs { uint16_t bin[HS_MAX_DIMS * 256]; };   // bin of byte value v in dimension d at [d * 256 + v], or HS_OUT_BIN; travels as a kernel argument

struct vp_hist_plan {
    int dims, cn;
    int channel[HS_MAX_DIMS];  // unused dimensions read channel 0 through a table of zeros
    int size[HS_MAX_DIMS];
    int step[HS_MAX_DIMS];     // counters between neighbouring bins of a dimension: the first dimension slowest; 0 for an unused one
    int total;                 // counters: the product of the sizes
    int in_lds;                // counters (histogram) or table (back-projection) live in LDS
    size_t lds_bytes;
    unsigned grid;
    vp_hist_tabs tabs;
};

// NULL: admitted; else the reason (VP_ERR_INVALID).  ranges: dims pairs (low, high).
static inline const char* vp_hist_refusal(int w, int h, int cn, size_t stride, int dims, const int32_t* channels, const int32_t* hist_size, const double* ranges)
{
    if (w < 1 || h < 1) return "hist: width and height must be at least 1";
    if (w > HS_MAX_SIDE || h > HS_MAX_SIDE) return "hist: width and height must be at most 4096";
    if (cn < 1 || cn > HS_MAX_CN) return "hist: 1 to 4 channels";
    if (stride < (size_t)w * cn) return "hist: the stride is below the row";
    if (dims < 1 || dims > HS_MAX_DIMS) return "hist: 1 to 3 dimensions";
    for (int d = 0; d < dims; d++) {
        if (channels[d] < 0 || channels[d] >= cn) return "hist: a channel index is outside the image's channels";
        if (hist_size[d] < 1 || hist_size[d] > HS_MAX_SIZE) return "hist: a histogram size must be 1 to 256";
        const double lo = ranges[2 * d], hi = ranges[2 * d + 1];
        if (!(lo < hi) || !isfinite(lo) || !isfinite(hi)) return "hist: a range needs finite ends with low < high";
    }
    return nullptr;
}

// a mask of mw x mh bytes in rows of mstride
static inline const char* vp_hist_mask_refusal(int w, int h, int mw, int mh, size_t mstride)
{
    if (mw != w || mh != h) return "hist: the mask must have the size of the image";
    if (mstride < (size_t)w) return "hist: the mask's stride is below its row";
    return nullptr;
}

// cv2's calcHistLookupTables_8u, uniform: a = size / (high - low), b = -a * low, bin(j) = floor(j * a + b), outside [0, size) -> no bin
static inline void vp_hist_make_tabs(int dims, const int32_t* hist_size, const double* ranges, vp_hist_tabs* T)
{
    for (int d = 0; d < HS_MAX_DIMS; d++) {
        if (d >= dims) {
            for (int j = 0; j < 256; j++) T->bin[d * 256 + j] = 0;
            continue;
        }
        const double lo = ranges[2 * d], hi = ranges[2 * d + 1];
        const double a = hist_size[d] / (hi - lo), b = -a * lo;
        for (int j = 0; j < 256; j++) {
            const double f = floor(j * a + b);
            T->bin[d * 256 + j] = (f >= 0 && f < hist_size[d]) ? (uint16_t)(int)f : (uint16_t)HS_OUT_BIN;
        }
    }
}

static inline unsigned vp_hist_grid(int w, int h, size_t lds_bytes)
{
    const size_t chunks = (size_t)((w + HS_PX - 1) / HS_PX) * h, want = (chunks + HS_THREADS - 1) / HS_THREADS;
    const size_t cap = lds_bytes > HS_LDS_BYTES / 4 ? HS_MAX_BLOCKS_BIG : HS_MAX_BLOCKS;
    return (unsigned)(want < cap ? want : cap);
}

// arguments as vp_hist_refusal admitted them; back_project: the LDS holds the folded byte table instead of the counters
static inline void vp_hist_make_plan(int w, int h, int cn, int dims, const int32_t* channels, const int32_t* hist_size, const double* ranges, int back_project,
                                     vp_hist_plan* P)
{
    P->dims = dims;
    P->cn = cn;
    P->total = 1;
    for (int d = 0; d < HS_MAX_DIMS; d++) {
        P->channel[d] = d < dims ? channels[d] : 0;
        P->size[d] = d < dims ? hist_size[d] : 1;
        P->total *= P->size[d];
    }
    for (int d = 0, below = P->total; d < HS_MAX_DIMS; d++) {
        below /= P->size[d];
        P->step[d] = d < dims ? below : 0;
    }
    vp_hist_make_tabs(dims, hist_size, ranges, &P->tabs);
    if (back_project) {
        P->in_lds = P->total <= HS_BP_LDS_BYTES;
        P->lds_bytes = HS_TAB_LDS_BYTES + (P->in_lds ? ((size_t)P->total + 3) / 4 * 4 : 0);
    } else {
        P->in_lds = P->total <= HS_HIST_LDS_BINS;
        P->lds_bytes = HS_TAB_LDS_BYTES + (P->in_lds ? (size_t)P->total * 4 : 0);
    }
    P->grid = vp_hist_grid(w, h, P->lds_bytes);
}

// ---- mean shift ----------------------------------------------------------------------------------------------------------------
// window (x, y, w, h) cut to the image: 0 when nothing is left (cv2's Rect & Rect gives the empty Rect())
static inline int vp_ms_clip(const int32_t* win, int cols, int rows, int32_t* out)
{
    const long long x0 = win[0] > 0 ? win[0] : 0, y0 = win[1] > 0 ? win[1] : 0;
    long long x1 = (long long)win[0] + win[2], y1 = (long long)win[1] + win[3];
    if (x1 > cols) x1 = cols;
    if (y1 > rows) y1 = rows;
    if (x1 <= x0 || y1 <= y0) { out[0] = out[1] = out[2] = out[3] = 0; return 0; }
    out[0] = (int32_t)x0; out[1] = (int32_t)y0; out[2] = (int32_t)(x1 - x0); out[3] = (int32_t)(y1 - y0);
    return 1;
}

static inline const char* vp_mean_shift_refusal(int w, int h, size_t stride, const int32_t* windows, int n)
{
    if (w < 1 || h < 1) return "mean shift: width and height must be at least 1";
    if (w > HS_MAX_SIDE || h > HS_MAX_SIDE) return "mean shift: width and height must be at most 4096";
    if (stride < (size_t)w) return "mean shift: the stride is below the row";
    if (n < 1 || n > HS_MS_MAX_WINDOWS) return "mean shift: 1 to 4096 windows";
    for (int i = 0; i < n; i++) {
        int32_t c[4];
        if (windows[4 * i + 2] <= 0 || windows[4 * i + 3] <= 0) return "mean shift: a window has a non-positive size";
        if (!vp_ms_clip(windows + 4 * i, w, h, c)) return "mean shift: a window is empty inside the image";
    }
    return nullptr;
}

// cv2's TermCriteria as meanShift reads it: eps2 = round_half_even(max(eps, 0)^2), never above what dx^2 + dy^2 can reach + 1
static inline int vp_ms_eps2(double eps)
{
    const double e = eps > 0 ? eps : 0, top = 2.0 * HS_MAX_SIDE * HS_MAX_SIDE + 1;
    const double e2 = e * e;
    return !(e2 < top) ? (int)top : (int)nearbyint(e2);
}
static inline int vp_ms_iters(int max_iter) { return max_iter < 1 ? 1 : (max_iter > HS_MS_MAX_ITER ? HS_MS_MAX_ITER : max_iter); }
