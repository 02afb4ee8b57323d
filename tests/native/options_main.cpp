// The options table (csrc/vp_options.h) on the host.  Per row: the default, whether a set is accepted (A) or refused (R) at min - 1,
// min, max and max + 1, and the value held after a refused set; that ids outside the table are refused; then the defaults under a
// getenv that answers for one of the five named variables at a time.  Built with -fsanitize=address,undefined and compared with
// the expected text by tests/test_options_host.py.
#include "vp_options.h"
#include <climits>
#include <cstdio>
#include <cstring>
#include <initializer_list>

static const char* g_name = nullptr;    // the one variable the fake environment holds, and its text
static const char* g_text = nullptr;
static const char* fake_getenv(const char* name) { return g_name && strcmp(name, g_name) == 0 ? g_text : nullptr; }
static const char* no_getenv(const char*) { return nullptr; }

static void print_all(const char* tag, const vp_options& o)
{
    printf("%s", tag);
    for (int id = 1; id < VP_OPT_COUNT; id++) printf(" %d", o.v[id]);
    printf("\n");
}

int main()
{
    printf("count=%d\n", VP_OPT_COUNT);
    for (int id = 1; id < VP_OPT_COUNT; id++) {
        const vp_option_row* r = vp_option_find(id);
        if (!r) { printf("row %d missing\n", id); return 1; }
        vp_options o;
        vp_options_defaults(&o, no_getenv);
        printf("row %d default=%d env=%s", id, o.v[id], r->env ? r->env : "-");
        // min - 1 and max + 1 in 64 bits: a bound at INT_MIN / INT_MAX has no value outside it to try ("-")
        const long long tries[4] = {(long long)r->min - 1, r->min, r->max, (long long)r->max + 1};
        for (int k = 0; k < 4; k++) {
            if (tries[k] < INT_MIN || tries[k] > INT_MAX) { printf(" -"); continue; }
            vp_options p;
            vp_options_defaults(&p, no_getenv);
            const bool ok = vp_options_set(&p, id, (int)tries[k]);
            printf(" %lld:%c:%d", tries[k], ok ? 'A' : 'R', p.v[id]);
        }
        printf("\n");
    }
    for (int id : {0, 12, 77, -1}) {
        vp_options o, before;
        vp_options_defaults(&o, no_getenv);
        before = o;
        const bool ok = vp_options_set(&o, id, 1);
        printf("id %d %c changed=%d\n", id, ok ? 'A' : 'R', memcmp(&o, &before, sizeof o) != 0);
    }
    vp_options o;
    vp_options_defaults(&o, no_getenv);
    print_all("env none:", o);
    struct { const char* name; const char* in_range; const char* out_of_range; } vars[5] = {
        {"VP_CHAIN_STREAMS", "3", "5"}, {"VP_CCL_LEVELS", "1", "3"}, {"VP_OPT_MEDIAN_MASK", "1", "2"}, {"VP_OPT_CLAHE_SPLIT", "64", "65"},
        {"VP_OPT_CCL_CROWDED", "2", "-1"}};
    for (const auto& v : vars)
        for (const char* text : {v.in_range, v.out_of_range, "abc"}) {
            g_name = v.name; g_text = text;
            vp_options_defaults(&o, fake_getenv);
            char tag[96];
            snprintf(tag, sizeof tag, "env %s=%s:", v.name, text);
            print_all(tag, o);
        }
    // a variable that is no row's is never asked for, and so changes nothing
    g_name = "VP_OPT_FLAT_OPS"; g_text = "0";
    vp_options_defaults(&o, fake_getenv);
    print_all("env VP_OPT_FLAT_OPS=0:", o);
    return 0;
}
