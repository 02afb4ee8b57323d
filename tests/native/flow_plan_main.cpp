// Host sweep of csrc/vp_flow_plan.h, built with -fsanitize=address,undefined by tests/test_flow_plan_host.py: every window side 3..63,
// image sides round every level boundary, maxLevel 0..15.  Asserts the level rule, the LDS layout and its limit, and that every index
// the kernel forms for the extreme positions the range test admits lands inside its level and inside its LDS region.  Prints one
// summary line; exits non-zero at the first invariant that breaks.
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "vp_flow_plan.h"

static long long g_plans = 0, g_levels = 0, g_indices = 0, g_refused = 0;
static size_t g_max_lds = 0;

#define CHECK(cond, ...)                                                                                                              \
    do {                                                                                                                              \
        if (!(cond)) {                                                                                                                \
            printf("FAILED %s: ", #cond);                                                                                             \
            printf(__VA_ARGS__);                                                                                                      \
            printf("\n");                                                                                                             \
            exit(1);                                                                                                                  \
        }                                                                                                                             \
    } while (0)

// BORDER_REFLECT_101 by its definition, for one reflection
static int reflect_once(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// one axis of one level: positions ip from -win to n - 1 pass the range test; the patch reads ip - 1 .. ip + win + 1
static void sweep_axis(int n, int win)
{
    std::vector<unsigned char> line((size_t)n, 1);          // the sanitizer sees every access
    for (int ip = -win; ip <= n - 1; ip++) {
        for (int k = -1; k <= win + 1; k++) {
            const int r = vp_lk_reflect(ip + k, n);
            CHECK(r >= 0 && r < n, "n %d win %d ip %d k %d -> %d", n, win, ip, k, r);
            // what the window itself reads (0 .. win) needs one reflection only; the Scharr taps' extra pixel is read only beside a
            // pixel inside the level, where it is one step outside at most
            if (k >= 0 && k <= win) CHECK(r == reflect_once(ip + k, n), "n %d win %d ip %d k %d: more than one reflection", n, win, ip, k);
            if (ip + k >= -1 && ip + k <= n) CHECK(r == reflect_once(ip + k, n), "n %d ip+k %d: a tap beside the level", n, ip + k);
            g_indices += line[(size_t)r];
        }
    }
    // and whatever an integer can be: the clamp holds
    const int wild[] = {-2147483647, -1000000, 1000000, 2147483647};
    for (int v : wild) {
        const int r = vp_lk_reflect(v, n);
        CHECK(r >= 0 && r < n, "n %d wild %d -> %d", n, v, r);
    }
}

static void sweep_plan(int w, int h, int ww, int wh, int max_level)
{
    const char* why = vp_lk_refusal(w, h, ww, wh, 7, max_level, 30, 0.01, 0, 1e-4);
    if (w <= ww || h <= wh) {
        CHECK(why != nullptr, "%d x %d win %d x %d admitted", w, h, ww, wh);
        CHECK(vp_lk_level_count(w, h, ww, wh, max_level) == 0, "a level exists");
        g_refused++;
        return;
    }
    CHECK(why == nullptr, "%d x %d win %d x %d level %d refused: %s", w, h, ww, wh, max_level, why);
    vp_lk_plan P;
    vp_lk_make_plan(w, h, ww, wh, 7, max_level, &P);
    g_plans++;
    CHECK(P.levels >= 1 && P.levels <= max_level + 1 && P.levels <= LK_MAX_LEVELS, "levels %d", P.levels);
    CHECK(P.levels == vp_lk_level_count(w, h, ww, wh, max_level), "count");
    int cw = w, ch = h;
    for (int l = 0; l < P.levels; l++) {
        CHECK(P.cols[l] == cw && P.rows[l] == ch, "level %d is %d x %d, want %d x %d", l, P.cols[l], P.rows[l], cw, ch);
        CHECK(cw > ww && ch > wh, "level %d is not larger than the window", l);
        cw = (cw + 1) / 2;
        ch = (ch + 1) / 2;
        g_levels++;
    }
    if (P.levels <= max_level) CHECK(!(cw > ww && ch > wh), "level %d exists and was left out", P.levels);    // the rule stopped it, not the request
    // LDS: three regions in order, none overlapping, every index of the kernel inside its own
    const size_t patch = (size_t)(ww + 3) * (wh + 3), deriv = (size_t)(ww + 1) * (wh + 1) * 4, win = (size_t)ww * wh * 6;
    CHECK(P.patch_w == ww + 3 && P.patch_h == wh + 3, "patch");
    CHECK(P.off_deriv >= patch && P.off_deriv % 4 == 0, "deriv offset");
    CHECK(P.off_win >= P.off_deriv + deriv && P.off_win % 2 == 0, "window offset");
    CHECK(P.lds_bytes >= P.off_win + win && P.lds_bytes <= 65536 && P.lds_bytes <= LK_LDS_BYTES, "lds %zu", P.lds_bytes);
    CHECK((size_t)(wh + 2) * P.patch_w + ww + 2 < patch, "the last Scharr tap is outside the patch");
    CHECK((size_t)wh * (ww + 1) + ww < (size_t)(ww + 1) * (wh + 1), "the last derivative is outside its region");
    CHECK(P.grid == 7u, "grid");
    if (P.lds_bytes > g_max_lds) g_max_lds = P.lds_bytes;
}

int main()
{
    // the level rule and the LDS layout: every window, image sides round every level boundary (side = (win + d) << l, give or take one)
    for (int ww = LK_MIN_WIN; ww <= LK_MAX_WIN; ww++) {
        const int wh = ww <= 33 ? ww + (ww % 3) * 10 : LK_MAX_WIN + LK_MIN_WIN - ww;       // square and oblong windows, both ways round
        for (int l = 0; l <= 6; l++)
            for (int d = -1; d <= 2; d++) {
                const int w = ((ww + d) << l) + (d & 1) - (l > 0), h = ((wh + 1) << l) + 3;
                if (w < 1 || w > LK_MAX_SIDE || h > LK_MAX_SIDE) continue;
                for (int max_level = 0; max_level < LK_MAX_LEVELS; max_level++) {
                    sweep_plan(w, h, ww, wh, max_level);
                    sweep_plan(h, w, wh, ww, max_level);
                }
            }
        sweep_plan(LK_MAX_SIDE, LK_MAX_SIDE, ww, ww, 15);
        sweep_plan(ww, 100, ww, ww, 3);           // level 0 not larger than the window
        sweep_plan(100, ww, ww, ww, 3);
    }
    // the reflection: every window on every line length a level can have just above it, and on long ones
    for (int win = LK_MIN_WIN; win <= LK_MAX_WIN; win++) {
        for (int n = win + 1; n <= win + 4; n++) sweep_axis(n, win);
        sweep_axis(2 * win + 1, win);
        sweep_axis(LK_MAX_SIDE, win);
    }
    // refusals
    CHECK(vp_lk_refusal(0, 10, 3, 3, 1, 0, 1, 0, 0, 0), "w 0");
    CHECK(vp_lk_refusal(4097, 10, 3, 3, 1, 0, 1, 0, 0, 0), "w 4097");
    CHECK(vp_lk_refusal(100, 100, 2, 3, 1, 0, 1, 0, 0, 0) && vp_lk_refusal(100, 100, 3, 64, 1, 0, 1, 0, 0, 0), "window");
    CHECK(vp_lk_refusal(100, 100, 3, 3, 0, 0, 1, 0, 0, 0) && vp_lk_refusal(100, 100, 3, 3, LK_MAX_POINTS + 1, 0, 1, 0, 0, 0), "n");
    CHECK(!vp_lk_refusal(100, 100, 3, 3, LK_MAX_POINTS, 15, 1, 0, 12, 0), "the largest admitted call");
    CHECK(vp_lk_refusal(100, 100, 3, 3, 1, -1, 1, 0, 0, 0) && vp_lk_refusal(100, 100, 3, 3, 1, 16, 1, 0, 0, 0), "max_level");
    CHECK(vp_lk_refusal(100, 100, 3, 3, 1, 0, 1, 0, 1, 0) && vp_lk_refusal(100, 100, 3, 3, 1, 0, 1, 0, 16, 0), "flags");
    CHECK(vp_lk_refusal(100, 100, 3, 3, 1, 0, 1, NAN, 0, 0) && vp_lk_refusal(100, 100, 3, 3, 1, 0, 1, 0, 0, INFINITY), "not finite");
    CHECK(vp_lk_max_count(-5) == 0 && vp_lk_max_count(101) == 100 && vp_lk_max_count(30) == 30, "max_count");
    CHECK(vp_lk_eps2(-1) == 0 && vp_lk_eps2(11) == 100 && vp_lk_eps2(0.5) == 0.25, "eps");
    CHECK(vp_lk_level_count(100, 90, 21, 21, 5) == 3, "100 x 90 with 21 x 21: 100, 50, 25");
    printf("plans %lld levels %lld indices %lld refused %lld max_lds %zu limit %d\n", g_plans, g_levels, g_indices, g_refused, g_max_lds, LK_LDS_BYTES);
    return 0;
}
