// The labelling plan (csrc/vp_ccl_plan.h) on the host: one line per (frame size, ccl_levels, ccl_mcap, environment) with every field
// vpk_ccl decides before its first launch, in the format of tests/golden/ccl_plan.txt (recorded from the dispatcher as it was
// before the plan had a header of its own).  Built with -fsanitize=address,undefined by tests/test_ccl_plan_host.py.
#include "vp_ccl_plan.h"
#include <cstdio>

static void line(const char* env, int h, int w, int levels, int mcap, const ccl_tuning& T)
{
    const ccl_plan P = ccl_make_plan(w, h, /* VP_CCL_BLOCK2X2 */ 0, levels, mcap, T);
    const ccl_geom& G = P.G;
    size_t cap1;
    const size_t lds1 = ccl_local_lds(G, cap1, T);
    printf("env=%s h=%d w=%d levels=%d mcap_in=%d : rows=%d ww=%d wb=%d nids=%u strips=%d gpr=%u magic=%u cap2=%zu rc=%zu tail_words=%zu lds2=%zu two_level=%d mcap=%d "
           "R3=%d strips3=%d ids3=%u ok3=%d tall=%d lds3a=%zu lds3b=%zu lds3c=%zu lds1=%zu cap1=%zu\n",
           env, h, w, levels, mcap, G.rows, G.ww, G.wb, G.nids, P.strips, P.gpr, P.magic, P.cap2, P.rc, P.tail_words, P.lds2, (int)P.two_level, P.mcap, P.P3.R, P.P3.strips,
           P.P3.ids, P.P3.ok, (int)P.c3_tall, P.lds3a, P.lds3b, P.lds3c, lds1, cap1);
}

int main()
{
    static const int hw[][2] = {{1, 1}, {7, 3}, {33, 65}, {97, 257}, {130, 1}, {1, 130}, {200, 420}, {1080, 1920}, {2160, 3840}, {40, 2500}, {70, 4096}, {35, 2049},
                                {16, 4160}, {8, 8200}};
    const ccl_tuning T0 = ccl_tuning_from_env();
    for (const auto& c : hw)
        for (int levels = 1; levels <= 2; levels++)
            for (int mcap : {-1, 0, 6}) line("-", c[0], c[1], levels, mcap, T0);
    setenv("VP_C3_IDS", "8192", 1);
    line("VP_C3_IDS=8192", 1080, 1920, 2, -1, ccl_tuning_from_env());
    unsetenv("VP_C3_IDS");
    setenv("VP_CL_ROWS", "16", 1);
    line("VP_CL_ROWS=16", 1080, 1920, 2, -1, ccl_tuning_from_env());
    return 0;
}
