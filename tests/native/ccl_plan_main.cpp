// The labelling plan (csrc/vp_ccl_plan.h) on the host: one line per (frame size, ccl_levels, ccl_mcap, environment) with every field
// vpk_ccl decides before its first launch, in the format of tests/golden/ccl_plan.txt (recorded from the dispatcher as it was
// before the plan had a header of its own).  Built with -fsanitize=address,undefined by tests/test_ccl_plan_host.py.
#include "vp_ccl_plan.h"
#include <cstdio>
#include <cstdlib>

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
    unsetenv("VP_CL_ROWS");
    // the shapes of tests/ccl_cases.py (masks on the two sides of every capacity) and the environment settings its child processes run under
    static const int hw2[][2] = {{65, 200}, {65, 64}, {40, 2112}, {704, 200}, {64, 200}, {64, 400}, {64, 640}, {8192, 64}, {8193, 64}, {20, 4096}, {1024, 64},
                                 {1026, 64}};
    for (const auto& c : hw2)
        for (int levels = 1; levels <= 2; levels++)
            for (int mcap : {-1, 0, 6}) line("-", c[0], c[1], levels, mcap, T0);
    struct tuned { const char* name; const char* value; int h, w, levels, mcap; };
    static const tuned tn[] = {{"VP_CCL3", "0", 65, 200, 2, -1},      {"VP_CCL3", "0", 64, 200, 2, -1},       {"VP_C3_IDS", "8192", 20, 4096, 2, -1},
                               {"VP_C3_IDS", "4096", 20, 4096, 2, -1}, {"VP_C3_IDS", "64", 1024, 64, 2, 0},   {"VP_C3_IDS", "64", 1026, 64, 2, 0},
                               {"VP_CL_ROWS", "8", 65, 200, 1, -1},    {"VP_CL_ROWS", "8", 65, 200, 2, -1},    {"VP_CL_ROWS", "8", 40, 2112, 1, -1},
                               {"VP_CL_ROWS", "8", 40, 2112, 2, -1},   {"VP_CL_ROWS", "16", 65, 200, 1, -1},   {"VP_CL_ROWS", "16", 65, 200, 2, -1},
                               {"VP_CL_ROWS", "16", 40, 2112, 1, -1},  {"VP_CL_ROWS", "16", 40, 2112, 2, -1},  {"VP_CL_CAP", "64", 65, 200, 1, -1},
                               {"VP_CL_CAP", "64", 65, 200, 2, -1}};
    for (const tuned& t : tn) {
        char env[64];
        snprintf(env, sizeof env, "%s=%s", t.name, t.value);
        setenv(t.name, t.value, 1);
        line(env, t.h, t.w, t.levels, t.mcap, ccl_tuning_from_env());
        unsetenv(t.name);
    }
    return 0;
}
