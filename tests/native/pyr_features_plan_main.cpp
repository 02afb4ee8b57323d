// Host sweep of the pyramid plan in csrc/vp_features_plan.h, built with -fsanitize=address,undefined by
// tests/test_pyr_features_plan_host.py: image sides round 31, round the 64 x 16 tile and round each level boundary, every number of
// levels and a range of budgets.  Asserts that every workspace region is positive, aligned and disjoint, that the levels' pixel ranges
// and tile ranges are disjoint and cover the selection grid and the score grid exactly once, and that the quotas sum to the budget.
// Prints one summary line; exits non-zero at the first invariant that breaks.
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <utility>
#include <vector>

#include "vp_features_plan.h"

static long long g_plans = 0, g_empty = 0, g_refused = 0, g_level_plans[FT_PYR_MAX_LEVELS + 1] = {0};
static size_t g_max_ws = 0;

#define CHECK(cond, ...)                                                                                                              \
    do {                                                                                                                              \
        if (!(cond)) {                                                                                                                \
            printf("FAILED %s: ", #cond);                                                                                             \
            printf(__VA_ARGS__);                                                                                                      \
            printf("\n");                                                                                                             \
            exit(1);                                                                                                                  \
        }                                                                                                                             \
    } while (0)

static void pyr_case(int w, int h, int levels, int budget)
{
    if (vp_pyr_refusal(w, h, (size_t)(w > 0 ? w : 0), levels, 20, budget)) { g_refused++; return; }
    vp_pyr_plan P;
    vp_pyr_make_plan(w, h, levels, budget, &P);
    const vp_pyr_table& T = P.T;
    CHECK(T.n_levels >= 0 && T.n_levels <= levels, "%d levels of %d", T.n_levels, levels);
    CHECK((T.n_levels == 0) == (w < FT_DESC_MIN_SIDE || h < FT_DESC_MIN_SIDE), "%d x %d gives %d levels", w, h, T.n_levels);
    g_level_plans[T.n_levels]++;
    if (!T.n_levels) { g_empty++; return; }
    // the levels: the size rule, the cut-off, and one more level would have been too small or too many
    int lw = w, lh = h;
    long long quota_sum = 0, area = 0;
    uint32_t px = 0, tiles = 0;
    for (int l = 0; l < T.n_levels; l++) {
        const vp_pyr_level& L = T.L[l];
        CHECK(L.w == lw && L.h == lh && lw >= FT_DESC_MIN_SIDE && lh >= FT_DESC_MIN_SIDE, "level %d is %d x %d, not %d x %d", l, L.w, L.h, lw, lh);
        CHECK(L.off == px && L.off % FT_SEL_BLOCK == 0, "level %d starts at pixel %u, not %u", l, L.off, px);
        CHECK(L.tile_begin == tiles && L.tiles_x >= 1 && P.tiles_y[l] >= 1, "level %d's tiles start at %u, not %u", l, L.tile_begin, tiles);
        CHECK((size_t)L.tiles_x * FT_TW >= (size_t)lw && (size_t)(L.tiles_x - 1) * FT_TW < (size_t)lw, "tiles_x %u for %d", L.tiles_x, lw);
        CHECK((size_t)P.tiles_y[l] * FT_TH >= (size_t)lh && (size_t)(P.tiles_y[l] - 1) * FT_TH < (size_t)lh, "tiles_y %u for %d", P.tiles_y[l], lh);
        const size_t a = (size_t)lw * lh, padded = (a + FT_SEL_BLOCK - 1) / FT_SEL_BLOCK * FT_SEL_BLOCK;
        px += (uint32_t)padded;
        tiles += L.tiles_x * P.tiles_y[l];
        quota_sum += L.quota;
        area += (long long)a;
        lw = (5 * lw + 3) / 6;
        lh = (5 * lh + 3) / 6;
    }
    CHECK(T.n_levels == levels || lw < FT_DESC_MIN_SIDE || lh < FT_DESC_MIN_SIDE, "a level of %d x %d was left out", lw, lh);
    CHECK(T.total_px == px && T.total_tiles == tiles && px % FT_SEL_BLOCK == 0, "totals %u px %u tiles", T.total_px, T.total_tiles);
    CHECK(quota_sum == budget, "the quotas sum to %lld, not %d", quota_sum, budget);
    for (int l = 1; l < T.n_levels; l++)
        CHECK((long long)T.L[l].quota == (long long)budget * ((long long)T.L[l].w * T.L[l].h) / area, "quota %u of level %d", T.L[l].quota, l);
    // every tile of the score grid belongs to exactly one level and one place in it
    if (tiles <= 4096) {
        std::vector<unsigned char> seen(tiles, 0);
        for (int l = 0; l < T.n_levels; l++)
            for (uint32_t ty = 0; ty < P.tiles_y[l]; ty++)
                for (uint32_t tx = 0; tx < T.L[l].tiles_x; tx++) {
                    const uint32_t t = T.L[l].tile_begin + ty * T.L[l].tiles_x + tx;
                    CHECK(t < tiles, "tile %u of %u", t, tiles);
                    seen[t]++;
                }
        for (uint32_t t = 0; t < tiles; t++) CHECK(seen[t] == 1, "tile %u is covered %d times", t, (int)seen[t]);
        // and the kernels' rule - the last level whose first tile is not after the block - finds that level
        for (uint32_t t = 0; t < tiles; t++) {
            int l = 0;
            for (int k = 1; k < FT_PYR_MAX_LEVELS; k++)
                if (k < T.n_levels && t >= T.L[k].tile_begin) l = k;
            const uint32_t lt = t - T.L[l].tile_begin;
            CHECK(lt < T.L[l].tiles_x * P.tiles_y[l], "tile %u falls outside level %d", t, l);
        }
    }
    // the selection: whole blocks and waves inside one level, the grids cover the padded pixels exactly
    CHECK(P.chunks * FT_CHUNK == px && (size_t)P.sel_blocks * FT_SEL_BLOCK == px, "chunks %zu blocks %u for %u px", P.chunks, P.sel_blocks, px);
    CHECK(P.scan_per_lane >= 1 && P.scan_per_lane * FT_SCAN_LANES >= P.chunks, "scan %zu", P.scan_per_lane);
    const size_t np = (size_t)(budget > 0 ? budget : 1);
    CHECK(P.cap == (size_t)budget && (size_t)P.desc_grid * FT_DESC_WAVES >= np && (size_t)(P.desc_grid - 1) * FT_DESC_WAVES < np, "describe grid %u for %d", P.desc_grid, budget);
    // the workspace: positive, aligned, disjoint, inside ws_bytes
    std::vector<std::pair<size_t, size_t>> regions = {
        {P.off_img, px}, {P.off_score, px}, {P.off_keep, px}, {P.off_blur, px}, {P.off_tmp, (size_t)w * h * 2}, {P.off_hist, (size_t)FT_PYR_HIST_BYTES},
        {P.off_gt, (P.chunks + 1) * 4}, {P.off_eq, (P.chunks + 1) * 4}, {P.off_epre, (P.chunks + 1) * 4}, {P.off_lxy, np * 12}, {P.off_val, np * 4}, {P.off_bin, np},
        {P.off_desc, np * FT_DESC_BYTES}};
    for (auto& r : regions) CHECK(r.second > 0 && r.first % 256 == 0 && r.first + r.second <= P.ws_bytes, "region at %zu of %zu bytes in %zu", r.first, r.second, P.ws_bytes);
    std::sort(regions.begin(), regions.end());
    for (size_t i = 1; i < regions.size(); i++)
        CHECK(regions[i - 1].first + regions[i - 1].second <= regions[i].first, "regions at %zu and %zu overlap", regions[i - 1].first, regions[i].first);
    if (P.ws_bytes > g_max_ws) g_max_ws = P.ws_bytes;
    g_plans++;
}

int main()
{
    std::vector<int> sides = {-1, 0, 1, 25, 29, 30, 31, 32, 33, 35, 36, 37, 38, 43, 44, 45, 52, 53, 54, 63, 64, 65, 66, 76, 77, 78, 91, 92, 93, 110, 111, 112, 127, 128, 129,
                              130, 131, 132, 133, 159, 160, 161, 191, 192, 193, 255, 256, 257, 1080, 1920, 4096, 8192, 8193, 65535, 65536};
    // sides round each level boundary: the smallest side s whose level l is still 31, and its neighbours
    for (int l = 1; l < FT_PYR_MAX_LEVELS; l++)
        for (int s = 31; s < 400; s++) {
            int v = s;
            for (int k = 0; k < l; k++) v = (5 * v + 3) / 6;
            if (v >= FT_DESC_MIN_SIDE) {
                for (int d = -1; d <= 1; d++) sides.push_back(s + d);
                break;
            }
        }
    const int budgets[] = {-1, 0, 1, 2, 3, 7, 100, 500, 2000, 10000, FT_MAX_POINTS, FT_MAX_POINTS + 1};
    for (int w : sides)
        for (int h : sides)
            for (int levels = 0; levels <= FT_PYR_MAX_LEVELS + 1; levels++)
                for (int b : budgets) pyr_case(w, h, levels, b);
    for (int l = 1; l <= FT_PYR_MAX_LEVELS; l++) CHECK(g_level_plans[l] > 0, "no plan with %d levels was swept", l);
    printf("plans %lld empty %lld refused %lld eight_levels %lld max_ws %zu\n", g_plans, g_empty, g_refused, g_level_plans[FT_PYR_MAX_LEVELS], g_max_ws);
    return 0;
}
