// The histogram plan (csrc/vp_hist_plan.h) swept on the host under the address and undefined-behaviour sanitizers: for every
// combination of histogram sizes round the two LDS limits and for image sides 1..4096 at the edges, the counters or the table are in
// LDS exactly when they fit, the LDS of a block stays within a compute unit's, the steps address every counter once and none outside,
// the grid is in bounds and the bin tables hold only bins of their dimension.  A simulated block walks the table through the steps
// into buffers of exactly the planned sizes, so the sanitizers see every index.  The mean-shift checks clip every window of a sweep
// into the image.  Prints one line of totals; exits non-zero at the first broken invariant.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "vp_hist_plan.h"

#define CHECK(cond)                                                                                                                      \
    do {                                                                                                                                 \
        if (!(cond)) {                                                                                                                   \
            std::printf("FAILED %s at w=%d h=%d cn=%d sizes=%d,%d,%d dims=%d bp=%d (line %d)\n", #cond, w, h, cn, s[0], s[1], s[2], dims, bp, __LINE__); \
            return 1;                                                                                                                    \
        }                                                                                                                                \
    } while (0)

static int check_one(int w, int h, int cn, int dims, const int32_t* s, int bp, size_t* max_lds, long* in_lds, long* in_mem)
{
    const int32_t channels[3] = {cn - 1, 0, cn / 2};
    const double ranges[6] = {0, 256, 10.5, 200.25, 0, 180};
    CHECK(vp_hist_refusal(w, h, cn, (size_t)w * cn, dims, channels, s, ranges) == nullptr);
    vp_hist_plan P;
    vp_hist_make_plan(w, h, cn, dims, channels, s, ranges, bp, &P);
    long long total = 1;
    for (int d = 0; d < dims; d++) total *= s[d];
    CHECK(P.total == total && P.dims == dims && P.cn == cn);
    const long long limit = bp ? HS_BP_LDS_BYTES : HS_HIST_LDS_BINS;
    CHECK(P.in_lds == (total <= limit));
    const size_t body = P.in_lds ? (bp ? ((size_t)total + 3) / 4 * 4 : (size_t)total * 4) : 0;
    CHECK(P.lds_bytes == HS_TAB_LDS_BYTES + body && P.lds_bytes <= HS_LDS_BYTES);
    if (P.lds_bytes > *max_lds) *max_lds = P.lds_bytes;
    *in_lds += P.in_lds;
    *in_mem += !P.in_lds;
    // the grid: at least one block, never more than the cap, and never more than there are chunks of HS_THREADS lanes
    const size_t chunks = (size_t)((w + HS_PX - 1) / HS_PX) * h;
    CHECK(P.grid >= 1 && P.grid <= (P.lds_bytes > HS_LDS_BYTES / 4 ? HS_MAX_BLOCKS_BIG : HS_MAX_BLOCKS) && (size_t)(P.grid - 1) * HS_THREADS < chunks);
    // the tables: a bin of the dimension or HS_OUT_BIN; an unused dimension is all zeros with step 0
    for (int d = 0; d < HS_MAX_DIMS; d++) {
        CHECK(P.channel[d] >= 0 && P.channel[d] < cn);
        for (int j = 0; j < 256; j++) {
            const int b = P.tabs.bin[d * 256 + j];
            if (d >= dims) CHECK(b == 0 && P.step[d] == 0);
            else CHECK(b == HS_OUT_BIN || b < s[d]);
        }
    }
    // a simulated block: the LDS image of exactly lds_bytes, every counter reached once through the steps
    std::vector<unsigned char> lds(P.lds_bytes);
    int* tab = reinterpret_cast<int*>(lds.data());
    for (int i = 0; i < HS_MAX_DIMS * 256; i++) {
        const int d = i >> 8, b = P.tabs.bin[i];
        tab[i] = b == HS_OUT_BIN ? HS_OUT_OFFSET : b * P.step[d];
    }
    std::vector<unsigned char> seen((size_t)total, 0);
    for (int b0 = 0; b0 < P.size[0]; b0++)
        for (int b1 = 0; b1 < P.size[1]; b1++)
            for (int b2 = 0; b2 < P.size[2]; b2++) {
                const long long idx = (long long)b0 * P.step[0] + (long long)b1 * P.step[1] + (long long)b2 * P.step[2];
                CHECK(idx >= 0 && idx < total);
                seen[(size_t)idx]++;
                if (P.in_lds) {
                    if (bp) lds[HS_TAB_LDS_BYTES + (size_t)idx] = 1;
                    else reinterpret_cast<unsigned*>(lds.data() + HS_TAB_LDS_BYTES)[idx] = 1;
                }
            }
    for (long long i = 0; i < total; i++) CHECK(seen[(size_t)i] == 1);
    // the worst sum that holds an outside offset stays negative
    CHECK((long long)HS_OUT_OFFSET + 2 * (total - 1) < 0);
    return 0;
}

int main()
{
    long admitted = 0, in_lds = 0, in_mem = 0, windows = 0;
    size_t max_lds = 0;
    // every combination of three sizes whose product lies within 64 of one of the two limits, both kinds of plan, plus the corners
    static const int sides[] = {1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 1023, 1024, 1025, 1920, 4095, 4096};
    const int ns = (int)(sizeof(sides) / sizeof(sides[0]));
    for (int a = 1; a <= 256; a++)
        for (int b = a; b <= 256; b++)
            for (int c = b; c <= 256; c++) {
                const long long t = (long long)a * b * c;
                const bool near_hist = t >= HS_HIST_LDS_BINS - 64 && t <= HS_HIST_LDS_BINS + 64, near_bp = t >= HS_BP_LDS_BYTES - 64 && t <= HS_BP_LDS_BYTES + 64;
                const bool corner = (a == 1 || a == 256) && (b == 1 || b == 256) && (c == 1 || c == 256);
                if (!near_hist && !near_bp && !corner) continue;
                int32_t s[3] = {c, a, b};                        // a leading 1 is a dimension less
                int dims = 3;
                if (a == 1 && b == 1) { dims = 1; s[1] = s[2] = 1; }
                else if (a == 1) { dims = 2; s[1] = b; s[2] = 1; }
                for (int bp = 0; bp <= 1; bp++) {
                    if (check_one(64, 48, 3, dims, s, bp, &max_lds, &in_lds, &in_mem)) return 1;
                    admitted++;
                }
            }
    // image sides at the edges, every channel count, a small and a large histogram
    for (int cn = 1; cn <= 4; cn++)
        for (int i = 0; i < ns; i++)
            for (int j = 0; j < ns; j++)
                for (int bp = 0; bp <= 1; bp++) {
                    const int32_t small[3] = {16, 1, 1}, big[3] = {180, 256, 1}, cube[3] = {32, 32, 32};
                    if (check_one(sides[i], sides[j], cn, 1, small, bp, &max_lds, &in_lds, &in_mem)) return 1;
                    if (check_one(sides[i], sides[j], cn, 2, big, bp, &max_lds, &in_lds, &in_mem)) return 1;
                    if (check_one(sides[i], sides[j], cn, 3, cube, bp, &max_lds, &in_lds, &in_mem)) return 1;
                    admitted += 3;
                }
    // refusals
    {
        const int32_t ch[3] = {0, 1, 2}, sz[3] = {8, 8, 8}, ch_bad[3] = {0, 3, 1}, ch_neg[3] = {-1, 0, 0}, sz0[3] = {8, 0, 8}, sz257[3] = {257, 8, 8};
        const double r[6] = {0, 256, 0, 256, 0, 256}, r_eq[6] = {0, 256, 5, 5, 0, 256}, r_rev[6] = {9, 1, 0, 256, 0, 256};
        int bad = 0;
        bad += vp_hist_refusal(9, 9, 3, 27, 3, ch, sz, r) != nullptr;
        bad += vp_hist_refusal(9, 9, 3, 27, 0, ch, sz, r) == nullptr;
        bad += vp_hist_refusal(9, 9, 3, 27, 4, ch, sz, r) == nullptr;
        bad += vp_hist_refusal(9, 9, 3, 27, 3, ch_bad, sz, r) == nullptr;
        bad += vp_hist_refusal(9, 9, 3, 27, 1, ch_neg, sz, r) == nullptr;
        bad += vp_hist_refusal(9, 9, 3, 27, 3, ch, sz0, r) == nullptr;
        bad += vp_hist_refusal(9, 9, 3, 27, 1, ch, sz257, r) == nullptr;
        bad += vp_hist_refusal(9, 9, 3, 27, 3, ch, sz, r_eq) == nullptr;
        bad += vp_hist_refusal(9, 9, 3, 27, 1, ch, sz, r_rev) == nullptr;
        bad += vp_hist_refusal(4097, 9, 1, 4097, 1, ch, sz, r) == nullptr;
        bad += vp_hist_refusal(9, 4097, 1, 9, 1, ch, sz, r) == nullptr;
        bad += vp_hist_refusal(0, 9, 1, 9, 1, ch, sz, r) == nullptr;
        bad += vp_hist_refusal(9, 9, 5, 45, 1, ch, sz, r) == nullptr;
        bad += vp_hist_refusal(9, 9, 3, 26, 1, ch, sz, r) == nullptr;
        bad += vp_hist_mask_refusal(9, 9, 9, 9, 9) != nullptr;
        bad += vp_hist_mask_refusal(9, 9, 8, 9, 9) == nullptr;
        bad += vp_hist_mask_refusal(9, 9, 9, 10, 9) == nullptr;
        bad += vp_hist_mask_refusal(9, 9, 9, 9, 8) == nullptr;
        if (bad) {
            std::printf("FAILED %d of the single refusals\n", bad);
            return 1;
        }
    }
    // mean shift: whatever is admitted clips to a window inside the image; the criteria stay in range
    for (int i = 0; i < ns; i++)
        for (int j = 0; j < ns; j++) {
            const int cols = sides[i], rows = sides[j];
            static const int32_t at[] = {-2147483647 - 1, -5000, -1, 0, 1, 63, 4095, 4096, 5000, 2147483647};
            static const int32_t len[] = {-1, 0, 1, 2, 64, 4096, 4097, 2147483647};
            for (int32_t x : at)
                for (int32_t y : at)
                    for (int32_t ww : len)
                        for (int32_t hh : len) {
                            const int32_t win[4] = {x, y, ww, hh};
                            int32_t c[4];
                            const bool ok = vp_mean_shift_refusal(cols, rows, (size_t)cols, win, 1) == nullptr;
                            const int inside = vp_ms_clip(win, cols, rows, c);
                            if (ok != (ww > 0 && hh > 0 && inside)) { std::printf("FAILED window refusal %d %d %d %d in %d x %d\n", x, y, ww, hh, cols, rows); return 1; }
                            if (inside && !(c[0] >= 0 && c[1] >= 0 && c[2] >= 1 && c[3] >= 1 && c[0] + c[2] <= cols && c[1] + c[3] <= rows)) {
                                std::printf("FAILED clip %d %d %d %d in %d x %d\n", x, y, ww, hh, cols, rows);
                                return 1;
                            }
                            windows += ok;
                        }
        }
    {
        const int32_t win[4] = {0, 0, 1, 1};
        int bad = 0;
        bad += vp_mean_shift_refusal(9, 9, 8, win, 1) == nullptr;
        bad += vp_mean_shift_refusal(9, 9, 9, win, 0) == nullptr;
        bad += vp_mean_shift_refusal(9, 9, 9, win, HS_MS_MAX_WINDOWS + 1) == nullptr;
        bad += vp_mean_shift_refusal(4097, 9, 4097, win, 1) == nullptr;
        bad += vp_ms_eps2(1.0) != 1 || vp_ms_eps2(-2.0) != 0 || vp_ms_eps2(1.5) != 2 || vp_ms_eps2(2.5) != 6 || vp_ms_eps2(1e300) != 2 * 4096 * 4096 + 1;
        bad += vp_ms_iters(-5) != 1 || vp_ms_iters(0) != 1 || vp_ms_iters(7) != 7 || vp_ms_iters(2147483647) != HS_MS_MAX_ITER;
        if (bad) {
            std::printf("FAILED %d of the mean-shift checks\n", bad);
            return 1;
        }
    }
    std::printf("admitted %ld in_lds %ld in_memory %ld windows %ld max_lds %zu limit %d\n", admitted, in_lds, in_mem, windows, max_lds, HS_LDS_BYTES);
    return 0;
}
