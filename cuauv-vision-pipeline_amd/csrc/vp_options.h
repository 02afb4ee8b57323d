// The context's options (VP_OPT_*, include/vp.h): one row per option with its range, its default and the environment variable that
// may override the default at vp_create.  Plain C++ - no HIP types - so that the whole table is checked without a GPU
// (tests/native/options_main.cpp).  vp_set_option and vp_create go through the two functions below and nothing else writes a value;
// a use site reads ctx->opt.v[VP_OPT_X].
#pragma once
#include <limits.h>
#include <stdlib.h>
#include "../../include/vp.h"

#define VP_OPT_COUNT 12        // ids 1..11; slot 0 is unused

struct vp_options { int v[VP_OPT_COUNT]; };

struct vp_option_row { int id, min, max, def; const char* env; };

constexpr vp_option_row vp_option_rows[] = {
    {VP_OPT_CHAIN_STREAMS, 1, 4, 1, "VP_CHAIN_STREAMS"},          // sub-batches of a chain run on this many internal streams
    {VP_OPT_CCL_LEVELS, 1, 2, 2, "VP_CCL_LEVELS"},                // 2: two-level labelling with the one-level kernels as fallback; 1: one-level only
    {VP_OPT_CCL_MERGE_CAP, -1, INT_MAX, -1, nullptr},             // components per frame the merge block accepts (-1: its LDS capacity); tests lower it to force the fallback
    {VP_OPT_FLAT_OPS, 0, 1, 1, nullptr},                          // 1: the per-operator kernels take their 16-px-per-lane forms when rows are packed and pointers aligned; 0: always the generic kernels (tests)
    {VP_OPT_HOUGH_LDS, 0, 1, 1, nullptr},                         // 1: Hough rows counted in LDS where they fit; 0: every vote is a global atomic
    {VP_OPT_HOUGH_CIRCLES_LDS, 0, 1, 1, nullptr},                 // 1: HoughCircles radius histograms in LDS where they fit; 0: always in device memory
    {VP_OPT_BLUR_ONEPASS, -1, 1, -1, nullptr},                    // -1 the measured choice, 1 the one-pass kernel wherever its tile fits, 0 always two passes
    {VP_OPT_MEDIAN_MASK, -1, 1, -1, "VP_OPT_MEDIAN_MASK"},        // -1 the measured choice, 1 the mask kernel for every mask it can serve, 0 never
    {VP_OPT_CLAHE_SPLIT, 0, 64, 0, "VP_OPT_CLAHE_SPLIT"},         // 0 the measured choice, n >= 1 that many blocks share one CLAHE tile's histogram
    {VP_OPT_CCL_CROWDED, 0, 2, 0, "VP_OPT_CCL_CROWDED"},          // 0 by the hint, 1 always the crowded-frame kernels, 2 always the one stand-in launch
    {VP_OPT_LABEL_MOMENTS_LDS, -1, 1, -1, nullptr},               // -1 the measured choice, 1 the block's LDS table wherever it fits, 0 always device atomics
};
static_assert(sizeof vp_option_rows / sizeof vp_option_rows[0] == VP_OPT_COUNT - 1, "one row per option");

static inline const vp_option_row* vp_option_find(int id)
{
    for (const vp_option_row& r : vp_option_rows)
        if (r.id == id) return &r;
    return nullptr;
}

// false (and nothing changed) for an unknown id or a value outside the row's range
static inline bool vp_options_set(vp_options* o, int id, int value)
{
    const vp_option_row* r = vp_option_find(id);
    if (!r || value < r->min || value > r->max) return false;
    o->v[r->id] = value;
    return true;
}

// the defaults, then the environment's overrides: read with atoi, a value outside the row's range is ignored
template <class Getenv> static inline void vp_options_defaults(vp_options* o, Getenv env)
{
    o->v[0] = 0;
    for (const vp_option_row& r : vp_option_rows) {
        o->v[r.id] = r.def;
        if (!r.env) continue;
        if (const char* s = env(r.env)) vp_options_set(o, r.id, atoi(s));
    }
}
