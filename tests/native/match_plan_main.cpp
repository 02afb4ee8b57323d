// The template-matching plan (csrc/vp_match_plan.h) swept on the host under the address and undefined-behaviour sanitizers: for every
// admitted (w, h, cn, tw, th, method) of the sweep the tile grid covers the result exactly, the chunks cover every template row and
// word once, a simulated block stays inside its LDS and the image, LDS stays within the plan's limit, and the workspace regions do not
// overlap; refused arguments are refused.  Prints one line of totals; exits non-zero at the first broken invariant.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "vp_match_plan.h"

#define CHECK(cond)                                                                                                              \
    do {                                                                                                                         \
        if (!(cond)) {                                                                                                           \
            std::printf("FAILED %s at w=%d h=%d cn=%d tw=%d th=%d method=%d (line %d)\n", #cond, w, h, cn, tw, th, method, __LINE__); \
            return 1;                                                                                                            \
        }                                                                                                                        \
    } while (0)

static int check_one(int w, int h, int cn, int tw, int th, int method, long* blocks)
{
    vp_match_plan P;
    vp_match_make_plan(w, h, cn, tw, th, method, &P);
    CHECK(P.rw == w - tw + 1 && P.rh == h - th + 1 && P.rw >= 1 && P.rh >= 1);
    // the grid covers the result exactly: the last tile starts inside it, the tiles reach its end
    CHECK((long)(P.grid_x - 1) * MT_TILE_W < P.rw && (long)P.grid_x * MT_TILE_W >= P.rw);
    CHECK((long)(P.grid_y - 1) * MT_TILE_H < P.rh && (long)P.grid_y * MT_TILE_H >= P.rh);
    // the packed template row holds the template's bytes, in whole groups of four words
    CHECK(P.twb == tw * cn && P.tpitch % 4 == 0 && P.tpitch * 4 >= P.twb && P.tpitch * 4 < P.twb + 16);
    // the chunks cover every template row and word once, none larger than what LDS was sized for
    std::vector<int> rows(th, 0), words(P.tpitch, 0);
    int nrc = 0, ncc = 0;
    for (int jc = 0; jc < th; jc += MT_CHUNK_ROWS, nrc++) {
        const int cr = th - jc < MT_CHUNK_ROWS ? th - jc : MT_CHUNK_ROWS;
        CHECK(cr >= 1 && cr <= P.chunk_rows);
        for (int r = 0; r < cr; r++) rows[jc + r]++;
    }
    for (int kc = 0; kc < P.tpitch; kc += MT_CHUNK_WORDS, ncc++) {
        const int cw = P.tpitch - kc < MT_CHUNK_WORDS ? P.tpitch - kc : MT_CHUNK_WORDS;
        CHECK(cw >= 4 && cw % 4 == 0 && cw <= P.chunk_words);
        for (int c = 0; c < cw; c++) words[kc + c]++;
        // what the last lane of a block reads from a patch row stays inside the staged part of the row
        const int pw = MT_LANES_X * cn + cw + MT_PATCH_SLACK, nw = ((MT_RX - 1) * cn) / 4;
        CHECK((MT_LANES_X - 1) * cn + (cw - 4) + 3 + nw + 1 < pw && pw <= P.patch_pitch);
    }
    for (int r = 0; r < th; r++) CHECK(rows[r] == 1);
    for (int c = 0; c < P.tpitch; c++) CHECK(words[c] == 1);
    CHECK(nrc == P.row_chunks && ncc == P.col_chunks && P.one_piece == (nrc == 1 && ncc == 1));
    CHECK(P.one_piece == (th <= MT_CHUNK_ROWS && P.tpitch <= MT_CHUNK_WORDS));
    // LDS: the patch, then the chunk between its zero rows, 16-byte aligned, within the limit
    CHECK(P.patch_rows == MT_TILE_H + P.chunk_rows - 1 && (MT_LANES_Y - 1) * MT_RY + P.chunk_rows + MT_RY - 2 < P.patch_rows);
    CHECK(P.templ_off % 4 == 0 && P.templ_off >= P.patch_rows * P.patch_pitch);
    CHECK(P.lds_bytes == ((size_t)P.templ_off + (size_t)(P.chunk_rows + 2 * (MT_RY - 1)) * P.chunk_words) * 4 && P.lds_bytes <= MT_LDS_BYTES);
    // the last block's furthest image byte: clamped by the kernel, so only the arithmetic must not overflow
    CHECK((long long)(P.grid_x - 1) * MT_TILE_W * cn + 4ll * (P.tpitch + MT_LANES_X * cn + MT_PATCH_SLACK) < (1ll << 31));
    // the window sums the method reads, and a workspace whose regions follow one another
    const int s2 = method != MT_CCORR && method != MT_CCOEFF, s1 = method == MT_CCOEFF || method == MT_CCOEFF_NORMED;
    CHECK(P.need_s2 == s2 && P.need_s1 == s1 && P.planes == s2 + s1 * cn && P.ipitch == w + 1);
    CHECK(P.off_stats == 0 && P.off_templ >= sizeof(vp_match_stats) && P.off_templ % 256 == 0 && P.off_integral % 256 == 0);
    CHECK(P.off_integral >= P.off_templ + (size_t)th * P.tpitch * 4 && P.ws_bytes >= P.off_integral + (size_t)P.planes * (h + 1) * (w + 1) * 4);
    *blocks += (long)P.grid_x * P.grid_y;
    return 0;
}

int main()
{
    static const int sides[] = {1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1920, 4096};
    const int ns = (int)(sizeof(sides) / sizeof(sides[0]));
    long admitted = 0, refused = 0, blocks = 0, chunked = 0;
    size_t max_lds = 0;
    for (int cn = 0; cn <= 5; cn++)
        for (int a = 0; a < ns; a++)
            for (int b = 0; b < ns; b++)
                for (int c = 0; c < ns; c++)
                    for (int d = 0; d < ns; d++) {
                        const int w = sides[a], h = sides[b], tw = sides[c], th = sides[d];
                        for (int method = -1; method <= 6; method += (method == 0 ? 4 : 1)) {      // -1, 0, 4, 5, 6
                            const char* why = vp_match_template_refusal(w, h, cn, (size_t)w * (cn > 0 ? cn : 1), tw, th, (size_t)tw * (cn > 0 ? cn : 1), method,
                                                                        w >= tw ? (size_t)(w - tw + 1) * 4 : 0);
                            const bool ok = cn >= 1 && cn <= 4 && tw <= w && th <= h && (long long)tw * th * cn <= 65536 && method >= 0 && method <= 5;
                            if (ok != (why == nullptr)) {
                                std::printf("FAILED refusal at w=%d h=%d cn=%d tw=%d th=%d method=%d: %s\n", w, h, cn, tw, th, method, why ? why : "admitted");
                                return 1;
                            }
                            if (!ok) {
                                refused++;
                                continue;
                            }
                            admitted++;
                            if (check_one(w, h, cn, tw, th, method, &blocks)) return 1;
                            vp_match_plan P;
                            vp_match_make_plan(w, h, cn, tw, th, method, &P);
                            chunked += !P.one_piece;
                            if (P.lds_bytes > max_lds) max_lds = P.lds_bytes;
                        }
                    }
    // the other refusals: sizes outside 1..4096, strides below their rows, a result stride that is not a multiple of 4
    int bad = 0;
    bad += vp_match_template_refusal(0, 5, 1, 8, 1, 1, 1, 0, 4) == nullptr;
    bad += vp_match_template_refusal(5, -1, 1, 8, 1, 1, 1, 0, 4) == nullptr;
    bad += vp_match_template_refusal(4097, 5, 1, 4097, 1, 1, 1, 0, 4097 * 4) == nullptr;
    bad += vp_match_template_refusal(5, 4097, 1, 5, 1, 1, 1, 0, 20) == nullptr;
    bad += vp_match_template_refusal(9, 9, 1, 9, 0, 3, 3, 0, 40) == nullptr;
    bad += vp_match_template_refusal(9, 9, 1, 9, 3, 0, 3, 0, 40) == nullptr;
    bad += vp_match_template_refusal(9, 9, 3, 26, 3, 3, 9, 0, 28) == nullptr;
    bad += vp_match_template_refusal(9, 9, 3, 27, 3, 3, 8, 0, 28) == nullptr;
    bad += vp_match_template_refusal(9, 9, 3, 27, 3, 3, 9, 0, 27) == nullptr;
    bad += vp_match_template_refusal(9, 9, 3, 27, 3, 3, 9, 0, 30) == nullptr;
    bad += vp_match_template_refusal(9, 9, 3, 27, 3, 3, 9, 0, 28) != nullptr;
    bad += vp_match_template_refusal(9, 9, 3, 40, 3, 3, 50, 5, 64) != nullptr;
    if (bad) {
        std::printf("FAILED %d of the single refusals\n", bad);
        return 1;
    }
    std::printf("admitted %ld refused %ld blocks %ld chunked %ld max_lds %zu limit %d\n", admitted, refused, blocks, chunked, max_lds, MT_LDS_BYTES);
    return 0;
}
