// The rule that chooses what the two-level labelling queues behind its merge (csrc/vp_ccl_hint.h), driven on the host: every line is
// "<case> <call>:<mode> ..." with mode L (LEAN) or F (FULL), one entry per call.  Built with -fsanitize=address,undefined and
// compared with the expected text by tests/test_ccl_hint_host.py.
#include "vp_ccl_hint.h"
#include <cstdio>
#include <cstring>
#include <vector>

static void run(const char* name, const std::vector<unsigned>& hints, int force, int streams)
{
    ccl_hint_state st;
    memset(&st, 0, sizeof st);              // a new context is zero-filled
    printf("%s", name);
    for (size_t i = 0; i < hints.size(); i++) printf(" %zu:%c", i + 1, ccl_hint_decide(st, hints[i], force, streams) == CCL_MODE_LEAN ? 'L' : 'F');
    printf("\n");
}

int main()
{
    printf("quiet=%d lean=%d full=%d\n", CCL_HINT_QUIET, CCL_MODE_LEAN, CCL_MODE_FULL);
    run("start", {0, 0, 0}, CCL_FORCE_AUTO, 1);
    run("hint_gives_full_at_once", {0, 3, 0}, CCL_FORCE_AUTO, 1);
    {   // one crowded hint, then 31 quiet ones stay FULL, the 32nd gives LEAN
        std::vector<unsigned> h = {1};
        for (int i = 0; i < 33; i++) h.push_back(0);
        run("quiet_32", h, CCL_FORCE_AUTO, 1);
    }
    {   // a crowded hint after 20 quiet ones restarts the count: 31 more quiet ones stay FULL, the 32nd gives LEAN
        std::vector<unsigned> h = {1};
        for (int i = 0; i < 20; i++) h.push_back(0);
        h.push_back(128);
        for (int i = 0; i < 33; i++) h.push_back(0);
        run("restart", h, CCL_FORCE_AUTO, 1);
    }
    run("two_streams", {0, 0, 1, 0}, CCL_FORCE_AUTO, 2);
    run("two_streams_forced_lean", {0, 0, 1, 0}, CCL_FORCE_LEAN, 2);
    run("forced_full", {0, 0, 1, 0}, CCL_FORCE_FULL, 1);
    run("forced_lean", {0, 5, 5, 0}, CCL_FORCE_LEAN, 1);
    {   // the state follows the hints under an override: back in automatic mode the crowded run is remembered
        ccl_hint_state st;
        memset(&st, 0, sizeof st);
        const int a = ccl_hint_decide(st, 2, CCL_FORCE_LEAN, 1), b = ccl_hint_decide(st, 0, CCL_FORCE_AUTO, 1);
        printf("override_then_auto 1:%c 2:%c\n", a == CCL_MODE_LEAN ? 'L' : 'F', b == CCL_MODE_LEAN ? 'L' : 'F');
    }
    return 0;
}
