// Host sweep of csrc/vp_features_plan.h, built with -fsanitize=address,undefined by tests/test_features_plan_host.py: image sides round
// every tile boundary for the FAST and describe plans, row counts round every block, split and cap boundary for the matcher.  Asserts
// that every grid and workspace region is positive, ordered and inside its limit, that the raster chunks and the scan cover the image,
// and that the matcher's splits cover every train row exactly once.  Prints one summary line; exits non-zero at the first invariant
// that breaks.
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "vp_features_plan.h"

static long long g_fast = 0, g_desc = 0, g_ham = 0, g_refused = 0, g_split_plans = 0;
static int g_max_splits = 0;
static size_t g_max_partial = 0;

#define CHECK(cond, ...)                                                                                                              \
    do {                                                                                                                              \
        if (!(cond)) {                                                                                                                \
            printf("FAILED %s: ", #cond);                                                                                             \
            printf(__VA_ARGS__);                                                                                                      \
            printf("\n");                                                                                                             \
            exit(1);                                                                                                                  \
        }                                                                                                                             \
    } while (0)

static void fast_case(int w, int h, int capacity)
{
    if (vp_fast_refusal(w, h, (size_t)w, 10, capacity)) { g_refused++; return; }
    vp_fast_plan P;
    vp_fast_make_plan(w, h, capacity, &P);
    const size_t npx = (size_t)w * h;
    CHECK(P.tiles_x >= 1 && P.tiles_y >= 1 && (size_t)P.tiles_x * FT_TW >= (size_t)w && (size_t)(P.tiles_x - 1) * FT_TW < (size_t)w, "w %d", w);
    CHECK((size_t)P.tiles_y * FT_TH >= (size_t)h && (size_t)(P.tiles_y - 1) * FT_TH < (size_t)h && P.tiles_y <= 65535, "h %d", h);
    CHECK(P.chunks >= 1 && P.chunks * FT_CHUNK >= npx && (P.chunks - 1) * FT_CHUNK < npx, "chunks %zu of %zu", P.chunks, npx);
    CHECK(P.sel_blocks >= 1 && (size_t)P.sel_blocks * FT_SEL_BLOCK >= npx && (size_t)(P.sel_blocks - 1) * FT_SEL_BLOCK < npx, "blocks %u", P.sel_blocks);
    CHECK(P.scan_per_lane >= 1 && P.scan_per_lane * FT_SCAN_LANES >= P.chunks, "scan %zu", P.scan_per_lane);
    CHECK(P.max_found == (size_t)(w - 6) * (h - 6) && P.out_cap <= (size_t)capacity && P.out_cap <= P.max_found, "cap %zu", P.out_cap);
    CHECK(P.off_score % 256 == 0 && P.off_keep >= P.off_score + npx && P.off_cnt >= P.off_keep + npx && P.off_xy >= P.off_cnt + (P.chunks + 1) * 4 &&
              P.off_val >= P.off_xy + P.out_cap * 8 && P.ws_bytes >= P.off_val + P.out_cap * 4 && P.ws_bytes > 0,
          "regions of %d x %d", w, h);
    CHECK(P.off_keep % 256 == 0 && P.off_cnt % 256 == 0 && P.off_xy % 256 == 0 && P.off_val % 256 == 0, "alignment");
    g_fast++;
}

static void describe_case(int w, int h, int n)
{
    if (vp_describe_refusal(w, h, (size_t)w, n)) { g_refused++; return; }
    vp_describe_plan P;
    vp_describe_make_plan(w, h, n, &P);
    const size_t npx = (size_t)w * h, np = (size_t)(n > 0 ? n : 1);
    CHECK(P.grid >= 1 && (size_t)P.grid * FT_DESC_WAVES >= np && (size_t)(P.grid - 1) * FT_DESC_WAVES < np, "grid %u for %d", P.grid, n);
    CHECK(P.off_tmp >= P.off_blur + npx && P.off_pts >= P.off_tmp + npx * 2 && P.off_desc >= P.off_pts + np * 8 && P.off_bin >= P.off_desc + np * FT_DESC_BYTES &&
              P.off_status >= P.off_bin + np && P.ws_bytes >= P.off_status + np,
          "regions of %d x %d, %d points", w, h, n);
    CHECK(P.off_blur % 256 == 0 && P.off_tmp % 256 == 0 && P.off_pts % 256 == 0 && P.off_desc % 256 == 0, "alignment");
    g_desc++;
}

static void hamming_case(int nq, int nt, int D)
{
    if (vp_hamming_refusal(nq, nt, D, (size_t)D, (size_t)D, 2, 0)) { g_refused++; return; }
    vp_hamming_plan_t P;
    vp_hamming_make_plan(nq, nt, D, &P);
    CHECK(P.words == D / 8 && P.words_padded >= P.words && P.words_padded < 2 * P.words + 1 && (P.words_padded & (P.words_padded - 1)) == 0 && P.words_padded <= 16,
          "words %d of %d", P.words_padded, P.words);
    CHECK(P.lds_bytes > 0 && P.lds_bytes <= 65536 && P.lds_bytes == (size_t)HM_TILE * P.words_padded * 8, "lds %zu", P.lds_bytes);
    CHECK(P.train_splits >= 1 && P.train_splits <= HM_TARGET_BLOCKS && P.split_rows >= HM_TILE && P.split_rows % HM_TILE == 0, "splits %d rows %d", P.train_splits,
          P.split_rows);
    if (nq > 0) CHECK(P.query_tiles >= 1 && (long long)P.query_tiles * HM_QB >= nq && (long long)(P.query_tiles - 1) * HM_QB < nq && P.query_tiles <= 65535 * 32, "tiles %d", P.query_tiles);
    if (nt > 0) CHECK((long long)(P.train_splits - 1) * P.split_rows < nt && (long long)P.train_splits * P.split_rows >= nt, "splits %d x %d rows for %d", P.train_splits, P.split_rows, nt);
    if (nt > 0 && D == 32) {
        // every train row belongs to exactly one split (the split rule does not look at D: one length walks the rows)
        std::vector<unsigned char> seen((size_t)nt, 0);
        for (int s = 0; s < P.train_splits; s++) {
            const long long r0 = (long long)s * P.split_rows, r1 = r0 + P.split_rows < nt ? r0 + P.split_rows : nt;
            CHECK(r0 < nt, "split %d of %d starts at %lld of %d rows", s, P.train_splits, r0, nt);
            for (long long r = r0; r < r1; r++) seen[(size_t)r]++;
        }
        for (int r = 0; r < nt; r++) CHECK(seen[(size_t)r] == 1, "row %d of %d is in %d splits", r, nt, (int)seen[(size_t)r]);
    }
    if (P.query_tiles >= HM_TARGET_BLOCKS || nt <= HM_MIN_SPLIT_ROWS) CHECK(P.train_splits == 1, "a needless split: nq %d nt %d", nq, nt);
    CHECK((P.train_splits > 1) == (P.partial_bytes > 0) && P.partial_bytes == (P.train_splits > 1 ? (size_t)P.train_splits * nq * 16 : 0), "partial %zu", P.partial_bytes);
    CHECK(P.partial_bytes <= ((size_t)8 << 20), "partial results of %zu bytes", P.partial_bytes);
    if (P.train_splits > 1) g_split_plans++;
    if (P.train_splits > g_max_splits) g_max_splits = P.train_splits;
    if (P.partial_bytes > g_max_partial) g_max_partial = P.partial_bytes;
    g_ham++;
}

int main()
{
    const int sides[] = {0, 6, 7, 8, 9, 15, 16, 17, 30, 31, 32, 63, 64, 65, 67, 127, 128, 129, 255, 256, 257, 1080, 1920, 4096, 16384, 65535, 65536};
    const int caps[] = {-1, 0, 1, 100, 1 << 20, 0x7fffffff};
    for (int w : sides)
        for (int h : sides) {
            for (int c : caps) fast_case(w, h, c);
            for (int n : {-1, 0, 1, 3, 4, 5, 63, 64, 65, 257, 10000, FT_MAX_POINTS, FT_MAX_POINTS + 1}) describe_case(w, h, n);
        }
    const int rows[] = {-1, 0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 1151, 1152, 1153, 2047, 2048, 2049, 10000, 65535, 65536, 65537,
                        100000, 130816, 131072, 131073, HM_MAX_ROWS, HM_MAX_ROWS + 1};
    for (int nq : rows)
        for (int nt : rows)
            for (int D : {0, 7, 8, 16, 24, 32, 40, 64, 72, 128, 136}) hamming_case(nq, nt, D);
    int8_t* pat = (int8_t*)malloc(FT_PATTERN_BYTES);
    CHECK(pat && vp_ft_build_pattern(pat) == 0, "the pattern");
    int worst = 0;
    for (int i = 0; i < FT_PATTERN_BYTES; i++) worst = abs(pat[i]) > worst ? abs(pat[i]) : worst;
    CHECK(worst <= FT_DESC_BORDER, "a steered coordinate of %d", worst);
    free(pat);
    printf("fast %lld describe %lld hamming %lld refused %lld split_plans %lld max_splits %d max_partial %zu pattern_reach %d\n", g_fast, g_desc, g_ham, g_refused,
           g_split_plans, g_max_splits, g_max_partial, worst);
    return 0;
}
