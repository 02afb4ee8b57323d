// The contour plan (csrc/vp_contours_plan.h) on the host: one line per case of contours_plan_cases.h with the two workspace totals and
// every field vpk_find_contours reads, in the format of tests/golden/contours_plan.txt (recorded from the dispatcher as it was before
// the plan had a header of its own).  What must hold for every admitted case is asserted here as well (check): exit status 1 and a
// line on stderr.  Built with -fsanitize=address,undefined by tests/test_contours_plan_host.py.
#include "vp_contours_plan.h"
#include "contours_plan_cases.h"
#include <cstdio>
#include <cstring>

static int failures = 0;
#define CHECK(c, cond)                                                                                                                       \
    do {                                                                                                                                     \
        if (!(cond)) { failures++; fprintf(stderr, "w=%d h=%d n=%d mode=%d mc=%d many=%d: %s\n", (c).w, (c).h, (c).n, (c).mode, (c).mc, (int)(c).many, #cond); } \
    } while (0)

static void check(const ct_case& c, const ct_plan& P, size_t ws, size_t tree_ws)
{
    // the round sequences fit k_ctm's flag slots: the refusal inside the plan is dead for every size the pixel bound admits
    CHECK(c, P.rounds >= 2 && P.rounds < CTM_SEQ);
    CHECK(c, P.tree ? (P.rounds_tree >= 2 && P.rounds_tree < 64) : P.rounds_tree == 0);
    // grids: at least one block, at most what the dispatcher has always capped them at
    CHECK(c, P.wgrid >= 1 && P.wgrid == (unsigned)((P.nwords + 255) / 256));
    CHECK(c, P.hgrid >= 1 && P.hgrid <= 1024 && P.hgrid <= (P.hcap + 255) / 256);
    CHECK(c, P.mg >= 32 && P.mg <= 1024 && P.sg >= 8 && P.sg <= 256);
    if (P.tree) {
        CHECK(c, P.nb >= 1 && P.tb >= 1 && P.jb >= 1 && P.jb <= 1024 && P.jb <= P.nb && P.jtb >= 1 && P.jtb <= 1024 && P.jtb <= P.tb);
        CHECK(c, (size_t)P.nb * 256 > (size_t)c.mc && (size_t)P.tb * 256 >= 2 * (size_t)c.mc + 2);
        CHECK(c, P.key_bits >= 1 && P.key_bits <= 31 && (c.mc >= (1 << 30) || ((unsigned)c.mc + 1u) >> P.key_bits == 0));
    }
    // the placement as vpk_find_contours does it, from any 256-aligned start, ends inside the region its caller wants; no array is empty
    CHECK(c, P.nws == (P.tree ? CTW_ALL : CTW_BASE));
    for (size_t start : {(size_t)0, (size_t)256, (size_t)1 << 20}) {
        size_t off = start;
        for (int i = 0; i < P.nws; i++) {
            CHECK(c, P.ws[i].name && P.ws[i].bytes > 0);
            off = ct_align(off);
            off += P.ws[i].bytes;
        }
        CHECK(c, off - start <= ws + (P.tree ? tree_ws : 0));
    }
    // what the kernels index the arrays with
    CHECK(c, P.ws[CTW_PARTSUM].bytes >= (size_t)P.wgrid * c.n * 4);
    CHECK(c, P.ws[CTW_CSUM].bytes >= ((P.hcap + 1023) / 1024 + 1) * 4 * c.n);
    CHECK(c, P.ws[CTW_HMAPS].bytes == P.words * 32 && P.ws[CTW_NODE].bytes == P.hcap * c.n * 8);
    if (P.tree) CHECK(c, P.ws[CTW_SORT].bytes == c.sort && strcmp(P.ws[CTW_SORT].name, "sort") == 0);
    CHECK(c, P.defer_big == 0 || (c.n == 1 && !c.many));
    CHECK(c, P.skip_above == (P.defer_big ? (unsigned)CTJ_LDS_HEADS : 0u));
}

static void check_hdr(int mc)
{
    for (int tree = 0; tree <= 1; tree++) {
        const ct_hdr_layout L = ct_hdr(mc, tree != 0);
        const bool ok = 16 == L.counts && L.counts < L.offsets && L.offsets < L.hier && L.hier <= L.is_hole && (tree ? L.hier < L.is_hole : L.hier == L.is_hole) &&
                        L.is_hole < L.bytes && L.counts % 4 == 0 && L.offsets % 4 == 0 && L.hier % 4 == 0 &&
                        L.bytes == 16 + (size_t)mc * 9 + (tree ? (size_t)mc * 16 : 0);
        if (!ok) { failures++; fprintf(stderr, "header layout mc=%d tree=%d\n", mc, tree); }
    }
}

static void line(const ct_case& c)
{
    const size_t ws = ct_ws_base_bytes(c.w, c.h, c.n, c.mc), tree_ws = ct_ws_tree_bytes(c.mc, c.sort);
    const ct_plan P = ct_make_plan(c.w, c.h, c.n, c.mode, c.method, c.mc, c.hier, c.mirror, c.many, c.defer, c.hint, c.sort);
    printf("w=%d h=%d n=%d mode=%d method=%d mc=%d hier=%d mirror=%d many=%d defer=%d hint=%u sort=%zu : ws=%zu tree_ws=%zu ", c.w, c.h, c.n, c.mode, c.method,
           c.mc, (int)c.hier, (int)c.mirror, (int)c.many, (int)c.defer, c.hint, c.sort, ws, tree_ws);
    if (P.status != VP_OK) { printf("status=%d why=%s\n", P.status, P.why); return; }
    printf("status=0 tree=%d mirror=%d hint_slots=%d seg_mode=%d defer_big=%d skip_above=%u nwords=%d words=%zu hcap=%zu wgrid=%u hgrid=%u mg=%u sg=%u "
           "rounds=%d rounds_tree=%d key_bits=%d nb=%u tb=%u jb=%u jtb=%u\n",
           (int)P.tree, (int)P.mirror, (int)P.hint_slots, P.seg_mode, P.defer_big, P.skip_above, P.nwords, P.words, P.hcap, P.wgrid, P.hgrid, P.mg, P.sg,
           P.rounds, P.rounds_tree, P.key_bits, P.nb, P.tb, P.jb, P.jtb);
    check(c, P, ws, tree_ws);
    check_hdr(c.mc);
}

int main()
{
    ct_each_case(line);
    // the form: forced off, forced on, by the last head count - read anew on every call
    bool forced = true;
    unsetenv("VP_CT_MANY");
    if (ct_want_many(CTJ_LDS_HEADS, &forced) || forced || !ct_want_many(CTJ_LDS_HEADS + 1, &forced) || forced) { failures++; fprintf(stderr, "form: by hint\n"); }
    setenv("VP_CT_MANY", "0", 1);
    if (ct_want_many(600000, &forced) || !forced) { failures++; fprintf(stderr, "form: forced off\n"); }
    setenv("VP_CT_MANY", "1", 1);
    if (!ct_want_many(0, &forced) || !forced || !ct_want_many(0)) { failures++; fprintf(stderr, "form: forced on\n"); }
    unsetenv("VP_CT_MANY");
    return failures ? 1 : 0;
}
