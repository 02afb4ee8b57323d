// Host arithmetic of the feature operators (vp_features.hip): FAST-9 corners, the steered 256-bit binary descriptor and the brute-force
// Hamming matcher.  The argument checks as this library admits them, the tiles and grids of every launch, the workspace of a call, the
// orientation tables, the rule that generates the descriptor's pattern and its 32 steered copies, and the matcher's split of the train
// set over blocks.  Plain C++ - no HIP types, no kernels - and a pure function of its arguments, like vp_flow_plan.h.  DESIGN.md
// section 4.31; tests/features_restate.py is the statement.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define FT_MAX_SIDE 65535            // rows and columns
#define FT_MAX_PIXELS (1 << 28)
#define FT_MAX_POINTS (1 << 20)      // points of one describe call

// ---- FAST-9 ------------------------------------------------------------------------------------------------------------------------
#define FT_FAST_MIN_SIDE 7           // one candidate: the ring has radius 3
#define FT_FAST_R 3
#define FT_TW 64                     // the score kernel's tile: FT_TW x FT_TH pixels per block of 256 lanes, the ring's halo round it in LDS
#define FT_TH 16
#define FT_LDS_PITCH (FT_TW + 2 * FT_FAST_R + 2)   // bytes between the staged rows (a multiple of 4)
#define FT_CHUNK 64                  // the selection walks the image in raster order, one wave per FT_CHUNK pixels: a wave's corners are
                                     // numbered by a ballot, the waves by a prefix sum over their counts, so the order is the raster's
#define FT_SEL_BLOCK 256             // lanes per block of the two selection launches (FT_SEL_BLOCK / FT_CHUNK waves)
#define FT_SCAN_LANES 1024           // the one block that turns the counts into offsets

struct vp_fast_plan {
    unsigned tiles_x, tiles_y;       // grid of the score launch
    size_t chunks;                   // waves of the selection = counters
    unsigned sel_blocks;             // grid of the count and the write launch
    size_t scan_per_lane;            // counters each lane of the scan block sums
    size_t max_found;                // candidates: (w - 6)(h - 6)
    size_t out_cap;                  // corners the device list holds: min(capacity, max_found)
    size_t off_score, off_keep, off_cnt, off_xy, off_val, ws_bytes;   // the workspace of a call, 256-byte aligned regions (the source of the host form comes on top)
};

static inline size_t vp_ft_align(size_t n) { return (n + 255) / 256 * 256; }

// NULL: admitted; else the reason (VP_ERR_INVALID).  What does not depend on pointers.
static inline const char* vp_fast_refusal(int w, int h, size_t stride, int threshold, int capacity)
{
    if (w < FT_FAST_MIN_SIDE || h < FT_FAST_MIN_SIDE) return "FAST: width and height must be at least 7";
    if (w > FT_MAX_SIDE || h > FT_MAX_SIDE) return "FAST: width and height must be at most 65535";
    if ((long long)w * h > FT_MAX_PIXELS) return "FAST: more than 2^28 pixels";
    if (stride < (size_t)w) return "FAST: the stride is below the row";
    if (threshold < 0 || threshold > 255) return "FAST: the threshold must be 0 to 255";
    if (capacity < 0) return "FAST: the capacity is negative";
    return nullptr;
}

// arguments as vp_fast_refusal admitted them
static inline void vp_fast_make_plan(int w, int h, int capacity, vp_fast_plan* P)
{
    const size_t npx = (size_t)w * h;
    P->tiles_x = (unsigned)((w + FT_TW - 1) / FT_TW);
    P->tiles_y = (unsigned)((h + FT_TH - 1) / FT_TH);
    P->chunks = (npx + FT_CHUNK - 1) / FT_CHUNK;
    P->sel_blocks = (unsigned)((npx + FT_SEL_BLOCK - 1) / FT_SEL_BLOCK);
    P->scan_per_lane = (P->chunks + FT_SCAN_LANES - 1) / FT_SCAN_LANES;
    P->max_found = (size_t)(w - 2 * FT_FAST_R) * (h - 2 * FT_FAST_R);
    P->out_cap = (size_t)capacity < P->max_found ? (size_t)capacity : P->max_found;
    size_t off = 0;
    P->off_score = off; off += vp_ft_align(npx);
    P->off_keep = off;  off += vp_ft_align(npx);
    P->off_cnt = off;   off += vp_ft_align((P->chunks + 1) * 4);
    P->off_xy = off;    off += vp_ft_align(P->out_cap * 8);
    P->off_val = off;   off += vp_ft_align(P->out_cap * 4);
    P->ws_bytes = off + 256;
}

static_assert(FT_LDS_PITCH % 4 == 0 && FT_SEL_BLOCK % FT_CHUNK == 0 && FT_TW * FT_TH == 4 * 256, "FAST: four pixels per lane of the score tile; whole waves per selection block");
static_assert(((size_t)FT_MAX_PIXELS + FT_SEL_BLOCK - 1) / FT_SEL_BLOCK < (1u << 31), "FAST: the selection grid fits a launch");

// ---- the steered binary descriptor -------------------------------------------------------------------------------------------------
#define FT_DESC_MIN_SIDE 31
#define FT_DESC_BORDER 15            // a described pixel is at least this far from every border: the disc and every steered test stay inside
#define FT_DISC_R2 225               // the orientation disc: dx dx + dy dy <= 225
#define FT_DISC_SIDE 31
#define FT_BINS 32
#define FT_PAIRS 256
#define FT_DESC_BYTES 32
#define FT_BASE_MAX 10               // |coordinate| of the base pattern
#define FT_PATTERN_BYTES (FT_BINS * FT_PAIRS * 4)
#define FT_FIX_BITS 14
#define FT_BLUR_K 7                  // B = GaussianBlur(I, (7, 7), 2)
#define FT_BLUR_SIGMA 2.0
#define FT_DESC_WAVES 4              // one wave per point, this many per block

// 16384 cos(2 pi k / 32) and 16384 sin(2 pi k / 32), rounded half away from zero.  None of the 64 real values lies within 0.037 of a half
// integer, so the rounding does not depend on the libm that evaluated them; tests/test_features_abi.py compares.
static const int32_t vp_ft_cos[FT_BINS] = {16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196, 0, -3196, -6270, -9102, -11585, -13623, -15137, -16069,
                                           -16384, -16069, -15137, -13623, -11585, -9102, -6270, -3196, 0, 3196, 6270, 9102, 11585, 13623, 15137, 16069};
static const int32_t vp_ft_sin[FT_BINS] = {0, 3196, 6270, 9102, 11585, 13623, 15137, 16069, 16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196,
                                           0, -3196, -6270, -9102, -11585, -13623, -15137, -16069, -16384, -16069, -15137, -13623, -11585, -9102, -6270, -3196};

static inline const char* vp_describe_refusal(int w, int h, size_t stride, int n)
{
    if (w < FT_DESC_MIN_SIDE || h < FT_DESC_MIN_SIDE) return "describe: width and height must be at least 31";
    if (w > FT_MAX_SIDE || h > FT_MAX_SIDE) return "describe: width and height must be at most 65535";
    if ((long long)w * h > FT_MAX_PIXELS) return "describe: more than 2^28 pixels";
    if (stride < (size_t)w) return "describe: the stride is below the row";
    if (n < 0) return "describe: the point count is negative";
    if (n > FT_MAX_POINTS) return "describe: at most 1048576 points";
    return nullptr;
}

struct vp_describe_plan {
    unsigned grid;                   // blocks of FT_DESC_WAVES waves
    size_t off_blur, off_tmp, off_pts, off_desc, off_bin, off_status, ws_bytes;   // as in vp_fast_plan
};

static inline void vp_describe_make_plan(int w, int h, int n, vp_describe_plan* P)
{
    const size_t npx = (size_t)w * h, np = (size_t)(n > 0 ? n : 1);
    P->grid = (unsigned)((np + FT_DESC_WAVES - 1) / FT_DESC_WAVES);
    size_t off = 0;
    P->off_blur = off;   off += vp_ft_align(npx);
    P->off_tmp = off;    off += vp_ft_align(npx * 2);        // the blur's 8.8 intermediate
    P->off_pts = off;    off += vp_ft_align(np * 8);
    P->off_desc = off;   off += vp_ft_align(np * FT_DESC_BYTES);
    P->off_bin = off;    off += vp_ft_align(np);
    P->off_status = off; off += vp_ft_align(np);
    P->ws_bytes = off + 256;
}

static inline int vp_ft_rdiv(int v) { return v < 0 ? -((-v + (1 << (FT_FIX_BITS - 1))) >> FT_FIX_BITS) : (v + (1 << (FT_FIX_BITS - 1))) >> FT_FIX_BITS; }

// The pattern: 256 pairs (ax, ay, bx, by) drawn by the stated generator, then their 32 steered copies, out[bin][pair][4].  Returns 0,
// or -1 when a steered coordinate leaves -15 .. 15 (it cannot: a base point is at most sqrt(200) from the centre).
static inline int vp_ft_build_pattern(int8_t* out)
{
    int base[FT_PAIRS][4];
    uint32_t s = 0x9E3779B9u;
    int have = 0;
    while (have < FT_PAIRS) {
        int c[4];
        for (int i = 0; i < 4; i++) {
            s = s * 1664525u + 1013904223u;
            const int d1 = (int)((s >> 16) % 11u);
            s = s * 1664525u + 1013904223u;
            const int d2 = (int)((s >> 16) % 11u);
            c[i] = d1 + d2 - FT_BASE_MAX;
        }
        if (c[0] == c[2] && c[1] == c[3]) continue;
        bool seen = false;
        for (int j = 0; j < have && !seen; j++)
            seen = (base[j][0] == c[0] && base[j][1] == c[1] && base[j][2] == c[2] && base[j][3] == c[3]) ||
                   (base[j][0] == c[2] && base[j][1] == c[3] && base[j][2] == c[0] && base[j][3] == c[1]);
        if (seen) continue;
        for (int i = 0; i < 4; i++) base[have][i] = c[i];
        have++;
    }
    for (int k = 0; k < FT_BINS; k++)
        for (int i = 0; i < FT_PAIRS; i++)
            for (int e = 0; e < 2; e++) {
                const int x = base[i][2 * e], y = base[i][2 * e + 1];
                const int xs = vp_ft_rdiv(x * vp_ft_cos[k] - y * vp_ft_sin[k]), ys = vp_ft_rdiv(x * vp_ft_sin[k] + y * vp_ft_cos[k]);
                if (xs < -FT_DESC_BORDER || xs > FT_DESC_BORDER || ys < -FT_DESC_BORDER || ys > FT_DESC_BORDER) return -1;
                out[((size_t)k * FT_PAIRS + i) * 4 + 2 * e] = (int8_t)xs;
                out[((size_t)k * FT_PAIRS + i) * 4 + 2 * e + 1] = (int8_t)ys;
            }
    return 0;
}

// the orientation sums stay in int32: 709 pixels of the disc, |offset| <= 15, values <= 255; the bin's score is taken in int64
static_assert(709ll * 15 * 255 < (1ll << 31) && 709ll * 15 * 255 * 16384 * 2 < (1ll << 62), "describe: a moment or a bin score overflows");
static_assert(FT_PAIRS == 4 * 64, "describe: four ballots of one wave give the 256 bits");

// ---- the scale pyramid (tests/pyr_features_restate.py is the statement) --------------------------------------
// Levels of a step of 1.2: w_l = (5 w_{l-1} + 3) / 6, each resized from the one before, kept while both sides are at least 31.  Every
// region of the workspace that holds one byte per pixel (the levels, their scores, the kept scores, the blurs) lays the levels out one
// after the other, each packed (stride = width) and starting at a multiple of FT_SEL_BLOCK pixels: a selection block of FT_SEL_BLOCK
// lanes, and each of its waves, lies inside one level, and the concatenated raster is in the order level, y, x.
#define FT_PYR_MAX_LEVELS 8
#define FT_PYR_MAX_PIXELS (1 << 26)  // of level 0
#define FT_PYR_NUM 5                 // w_l = (FT_PYR_NUM w + FT_PYR_DEN / 2) / FT_PYR_DEN
#define FT_PYR_DEN 6

struct vp_pyr_level {
    uint32_t off;                    // first pixel of the level in every per-pixel region, a multiple of FT_SEL_BLOCK
    int32_t w, h;
    uint32_t quota;                  // q_l: the corners the level may keep
    uint32_t tile_begin, tiles_x;    // the level's FT_TW x FT_TH tiles are tile_begin .. tile_begin + tiles_x tiles_y - 1 of the score grid
};

struct vp_pyr_table {                // passed to the kernels by value
    int32_t n_levels;
    uint32_t total_px;               // padded pixels of all levels: a multiple of FT_SEL_BLOCK
    uint32_t total_tiles;            // grid of the score launch
    vp_pyr_level L[FT_PYR_MAX_LEVELS];
};

struct vp_pyr_plan {
    vp_pyr_table T;
    uint32_t tiles_y[FT_PYR_MAX_LEVELS];
    size_t chunks;                   // waves of the selection = counters of each of the three arrays: total_px / FT_CHUNK
    unsigned sel_blocks;             // grid of the three selection launches: total_px / FT_SEL_BLOCK
    size_t scan_per_lane;
    size_t cap;                      // max_points
    unsigned desc_grid;              // blocks of FT_DESC_WAVES waves for cap points
    size_t off_img, off_score, off_keep, off_blur, off_tmp, off_hist, off_gt, off_eq, off_epre, off_lxy, off_val, off_bin, off_desc, ws_bytes;
};
#define FT_PYR_HIST_BYTES (FT_PYR_MAX_LEVELS * 256 * 4 + FT_PYR_MAX_LEVELS * 8)   // the histograms, then (cutoff score, equal-score corners kept) per level

static inline const char* vp_pyr_refusal(int w, int h, size_t stride, int levels, int threshold, int max_points)
{
    if (w < 1 || h < 1) return "pyramid features: width and height must be at least 1";
    if (w > FT_MAX_SIDE || h > FT_MAX_SIDE) return "pyramid features: width and height must be at most 65535";
    if ((long long)w * h > FT_PYR_MAX_PIXELS) return "pyramid features: more than 2^26 pixels";
    if (stride < (size_t)w) return "pyramid features: the stride is below the row";
    if (levels < 1 || levels > FT_PYR_MAX_LEVELS) return "pyramid features: levels must be 1 to 8";
    if (threshold < 0 || threshold > 255) return "pyramid features: the threshold must be 0 to 255";
    if (max_points < 0) return "pyramid features: max_points is negative";
    if (max_points > FT_MAX_POINTS) return "pyramid features: at most 1048576 points";
    return nullptr;
}

// arguments as vp_pyr_refusal admitted them.  T.n_levels may be 0 (a side below 31): then nothing else is meaningful.
static inline void vp_pyr_make_plan(int w, int h, int levels, int max_points, vp_pyr_plan* P)
{
    vp_pyr_table& T = P->T;
    T.n_levels = 0;
    T.total_px = T.total_tiles = 0;
    long long area = 0;
    int lw = w, lh = h;
    for (int l = 0; l < levels && lw >= FT_DESC_MIN_SIDE && lh >= FT_DESC_MIN_SIDE; l++) {
        vp_pyr_level& L = T.L[l];
        L.off = T.total_px;
        L.w = lw;
        L.h = lh;
        L.tile_begin = T.total_tiles;
        L.tiles_x = (uint32_t)((lw + FT_TW - 1) / FT_TW);
        P->tiles_y[l] = (uint32_t)((lh + FT_TH - 1) / FT_TH);
        T.total_tiles += L.tiles_x * P->tiles_y[l];
        T.total_px += (uint32_t)(((size_t)lw * lh + FT_SEL_BLOCK - 1) / FT_SEL_BLOCK * FT_SEL_BLOCK);
        area += (long long)lw * lh;
        T.n_levels = l + 1;
        lw = (FT_PYR_NUM * lw + FT_PYR_DEN / 2) / FT_PYR_DEN;
        lh = (FT_PYR_NUM * lh + FT_PYR_DEN / 2) / FT_PYR_DEN;
    }
    long long rest = max_points;
    for (int l = 1; l < T.n_levels; l++) {
        T.L[l].quota = (uint32_t)((long long)max_points * ((long long)T.L[l].w * T.L[l].h) / area);
        rest -= T.L[l].quota;
    }
    if (T.n_levels) T.L[0].quota = (uint32_t)rest;
    const size_t px = T.total_px, np = (size_t)(max_points > 0 ? max_points : 1);
    P->chunks = px / FT_CHUNK;
    P->sel_blocks = (unsigned)(px / FT_SEL_BLOCK);
    P->scan_per_lane = (P->chunks + FT_SCAN_LANES - 1) / FT_SCAN_LANES;
    P->cap = (size_t)max_points;
    P->desc_grid = (unsigned)((np + FT_DESC_WAVES - 1) / FT_DESC_WAVES);
    size_t off = 0;
    P->off_img = off;   off += vp_ft_align(px);
    P->off_score = off; off += vp_ft_align(px);
    P->off_keep = off;  off += vp_ft_align(px);
    P->off_blur = off;  off += vp_ft_align(px);
    P->off_tmp = off;   off += vp_ft_align((size_t)w * h * 2);       // the blur's 8.8 intermediate, one level at a time: level 0 is the largest
    P->off_hist = off;  off += vp_ft_align(FT_PYR_HIST_BYTES);
    P->off_gt = off;    off += vp_ft_align((P->chunks + 1) * 4);
    P->off_eq = off;    off += vp_ft_align((P->chunks + 1) * 4);
    P->off_epre = off;  off += vp_ft_align((P->chunks + 1) * 4);
    P->off_lxy = off;   off += vp_ft_align(np * 12);
    P->off_val = off;   off += vp_ft_align(np * 4);
    P->off_bin = off;   off += vp_ft_align(np);
    P->off_desc = off;  off += vp_ft_align(np * FT_DESC_BYTES);
    P->ws_bytes = off + 256;
}

// A level is at most the one before, so all levels hold at most FT_PYR_MAX_LEVELS times level 0's padded pixels: the offsets fit 32
// bits, the selection grid fits a launch, and the workspace (four bytes a pixel, the 16-bit intermediate, three counters a wave and the
// point lists) stays far inside size_t.
#define FT_PYR_PX_BOUND ((unsigned long long)FT_PYR_MAX_LEVELS * (FT_PYR_MAX_PIXELS + FT_SEL_BLOCK))
static_assert(FT_PYR_PX_BOUND < (1ull << 32) && FT_PYR_PX_BOUND / FT_SEL_BLOCK < (1ull << 31), "pyramid: a pixel offset leaves 32 bits or the selection grid a launch");
static_assert(FT_PYR_PX_BOUND / (FT_TW * FT_TH) + FT_PYR_MAX_LEVELS * 2ull * (FT_MAX_SIDE / FT_TH + 1 + FT_MAX_SIDE / FT_TW + 1) < (1ull << 31), "pyramid: the score grid fits a launch");
static_assert(4 * FT_PYR_PX_BOUND + 2ull * FT_PYR_MAX_PIXELS + 3 * (FT_PYR_PX_BOUND / FT_CHUNK + 1) * 4 + (unsigned long long)FT_MAX_POINTS * 64 + (1ull << 20) < (1ull << 40) &&
                  sizeof(size_t) >= 8,
              "pyramid: the workspace stays inside size_t");
static_assert((long long)FT_MAX_POINTS * FT_PYR_MAX_PIXELS < (1ll << 62), "pyramid: a quota's product stays inside 64 bits");
static_assert(FT_SEL_BLOCK == 256, "pyramid: a selection block owns one 256-bin histogram, a lane a bin");

// ---- brute-force Hamming matcher ---------------------------------------------------------------------------------------------------
#define HM_MIN_D 8
#define HM_MAX_D 128
#define HM_MAX_ROWS (1 << 20)        // queries, and train rows
#define HM_QB 256                    // queries per block: a lane owns one query in registers
#define HM_TILE 128                  // train rows staged in LDS at a time (16 KiB at D = 128)
#define HM_TARGET_BLOCKS 512         // two blocks for each of the 256 CUs: a reasoned figure, not a measured one
#define HM_MIN_SPLIT_ROWS 1024       // below this a further block costs more in its partial result and the merge than it saves: reasoned, not measured
#define HM_NONE 0x7fffffff           // "no neighbour yet" in a partial result

struct vp_hamming_plan_t {
    int words;                       // D / 8
    int words_padded;                // the next power of two: what the kernel keeps (the padding is zero on both sides, so distances do not change)
    int query_tiles, train_splits;   // grid x, y
    int split_rows;                  // train rows of one split, a multiple of HM_TILE; the last split takes what is left
    size_t lds_bytes;
    size_t partial_bytes;            // train_splits > 1: [split][query][4] int32 (d0, i0, d1, i1)
};

static inline const char* vp_hamming_refusal(int nq, int nt, int D, size_t qstride, size_t tstride, int k, int cross_check)
{
    if (nq < 0 || nt < 0) return "hamming: a row count is negative";
    if (nq > HM_MAX_ROWS || nt > HM_MAX_ROWS) return "hamming: at most 1048576 rows";
    if (D < HM_MIN_D || D > HM_MAX_D || D % 8) return "hamming: the descriptor length must be a multiple of 8 from 8 to 128";
    if (qstride < (size_t)D || tstride < (size_t)D) return "hamming: a stride is below the row";
    if (qstride % 8 || tstride % 8) return "hamming: the strides must be multiples of 8";
    if (k < 1 || k > 2) return "hamming: k must be 1 or 2";
    if (cross_check && k != 1) return "hamming: cross-check goes with k = 1";
    return nullptr;
}

// nq, nt >= 0 and D as vp_hamming_refusal admitted them
static inline void vp_hamming_make_plan(int nq, int nt, int D, vp_hamming_plan_t* P)
{
    P->words = D / 8;
    int wp = 1;
    while (wp < P->words) wp *= 2;
    P->words_padded = wp;
    P->query_tiles = nq > 0 ? (nq + HM_QB - 1) / HM_QB : 0;
    int splits = 1;
    if (P->query_tiles > 0 && P->query_tiles < HM_TARGET_BLOCKS) {
        const int want = (HM_TARGET_BLOCKS + P->query_tiles - 1) / P->query_tiles, most = (nt + HM_MIN_SPLIT_ROWS - 1) / HM_MIN_SPLIT_ROWS;
        splits = want < most ? want : most;
        if (splits < 1) splits = 1;
    }
    int rows = nt > 0 ? (nt + splits - 1) / splits : HM_TILE;
    rows = (rows + HM_TILE - 1) / HM_TILE * HM_TILE;
    P->split_rows = rows;
    P->train_splits = nt > 0 ? (nt + rows - 1) / rows : 1;
    P->lds_bytes = (size_t)HM_TILE * wp * 8;
    P->partial_bytes = P->train_splits > 1 ? (size_t)P->train_splits * nq * 16 : 0;
}

static_assert((size_t)HM_TILE * (HM_MAX_D / 8) * 8 <= 65536, "hamming: the staged tile is below the 64 KiB a kernel gets without asking");
static_assert((HM_MAX_ROWS + HM_QB - 1) / HM_QB <= 65535 * 32 && HM_TARGET_BLOCKS <= 65535, "hamming: the grid fits a launch");
