// Host arithmetic of the labelling dispatch (vpk_ccl, vp_ccl.hip): which path a frame size takes, how many strips, how much dynamic
// LDS each kernel gets and which instantiation runs.  Plain C++ - no HIP types, no kernels - so that the whole plan is checked
// without a GPU (tests/native/ccl_plan_main.cpp against tests/golden/ccl_plan.txt).  The two structs that travel to the kernels as
// arguments, ccl_geom and c3_plan, live here as well.
#pragma once
#include <stddef.h>
#include <stdlib.h>
#include <algorithm>

typedef unsigned long long u64;
typedef unsigned int u32;

#define CL_ROWS 32             // largest strip height of the strip-local pass; G.rows is the one in use
#define WR_ROWS 4              // rows a block of the label-write kernels streams
#define C2_MCAP 2048           // two-level path (vp_ccl2.inl): strip components of one frame held in the merge block's LDS
#define C2_MAXSTRIPS 256
#define C3_IDS 16384           // crowded frames (vp_ccl3.inl): most segment ids per strip = entries of the LDS union-find (1080p: 16 rows = 15,360; VP_C3_IDS=8192: 8 rows)
#define C3_ACC 2304            // local components whose statistics are accumulated per pass over the strip (the labelling launch has a CU's LDS to itself either way: one pass for raw noise at 10 % and 50 %)
#define C3_LIGHT_ROOTS 1024    // strips with at most this many local roots are labelled by the LIGHT instantiation of k_ccl3_label: tables for that many roots
#define C3_LIGHT_ACC 768       // ... and accumulators for that many per pass: ~72 KB of LDS, two blocks per CU hide each other's fixed latencies
#define C3_MAX_STRIPS 512      // per-strip root counts of a frame are scanned in LDS by every block of the later launches
#define C3_STATE_BYTES 48      // sizeof(c3_state), as the workspace is carved

struct ccl_geom {
    int w, h, ww, wb, numbering;
    u32 nids;   // multiple of 128
    u32 nw32;   // nids / 32
    int rows;   // rows per strip of the strip-local pass: 32, or 16 for wide frames (see ccl_make_geom)
    int invert; // label the zero pixels instead (background regions, for hole borders)
    int conn4;  // 4-connectivity (background of an 8-connected foreground)
};

struct c3_plan {
    int R, strips;             // rows per strip (even), strips per frame
    u32 ids;                   // R * wb: multiple of 32, <= C3_IDS
    int ok;
};

// What the environment may tune, with the defaults; ccl_tuning_from_env is read once per process (ccl_env_tuning, vp_ccl.hip).
struct ccl_tuning {
    u32 c3_ids = C3_IDS;       // VP_C3_IDS: segment ids per crowded-frame strip (larger values count as C3_IDS)
    bool c3_off = false;       // VP_CCL3=0: handed-over frames go to the one-level kernels
    int lgrid = 16;            // VP_C3_LGRID: blocks per CU of k_ccl3_link
    int bgrid = 64;            // VP_C3_BGRID: ... of k_ccl3_bound (items differ a lot in cost, the dispatcher balances)
    int agrid = 2;             // VP_C3_AGRID: ... of the heavy k_ccl3_label
    int agrid_light = 4;       // VP_C3_AGRID_LIGHT: ... of the light one
    int cl_rows = 0;           // VP_CL_ROWS: strip height of the strip-local pass (8, 16 or 32 where the bitmap slices allow; 0: by geometry)
    size_t cl_cap = 0;         // VP_CL_CAP: segments per strip of k_ccl_local (>= 64 and below the default; 0: the default)
};

static inline ccl_tuning ccl_tuning_from_env()
{
    ccl_tuning T;
    auto num = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
    T.c3_ids = (u32)num("VP_C3_IDS", C3_IDS);
    T.c3_off = num("VP_CCL3", 1) == 0;
    T.lgrid = num("VP_C3_LGRID", T.lgrid); T.bgrid = num("VP_C3_BGRID", T.bgrid);
    T.agrid = num("VP_C3_AGRID", T.agrid); T.agrid_light = num("VP_C3_AGRID_LIGHT", T.agrid_light);
    T.cl_rows = num("VP_CL_ROWS", 0);
    T.cl_cap = (size_t)num("VP_CL_CAP", 0);
    return T;
}

static inline size_t ccl_nids(int w, int h)   // segment ids of a frame (vp_ccl_nids)
{
    const size_t wb = (size_t)(w + 1) / 2, hb = (size_t)(h + 1) / 2;
    return (2 * hb * wb + 127) / 128 * 128;
}

// strips of the strip-local pass never exceed h / 8 + 1 (ccl_make_geom picks 8, 16 or 32 rows)
static inline size_t c2_strips_max(int h) { return (size_t)(h + 7) / 8; }
static inline size_t c3_strips_cap(int h) { return (size_t)(h + 1) / 2 + 2; }   // vp_ccl3.inl: strips of at least 2 rows, + 1 boundary slot

static inline void ccl_make_geom(ccl_geom& G, int w, int h, int numbering, int invert, int conn4, const ccl_tuning& T)
{
    G.w = w; G.h = h; G.ww = (w + 63) / 64 /* = vp_ww(w), vp_internal.h */; G.wb = (w + 1) / 2; G.numbering = numbering;
    G.nids = (u32)ccl_nids(w, h);
    G.nw32 = G.nids / 32;
    G.invert = invert; G.conn4 = conn4;
    // Strip height of the strip-local pass.  A block's time grows faster than its strip (64 rows: 75 us, 32: 53 us at 1080p), and
    // wide rows make strips heavy: at 4K (60 words per row) 16-row strips take k_ccl_local from 116 to 44 us for +4 us of
    // boundary unions; at 1080p the two cancel.  16 rows need ceil(w/2) even (bitmap slices must not share a word).
    G.rows = (G.ww > 32 && (G.wb % 2) == 0) ? 16 : 32;
    const int r = T.cl_rows;
    if ((r == 8 || r == 16 || r == 32) && ((u32)r * (u32)G.wb) % 32u == 0) G.rows = r;
}

// LDS of the strip-local kernels: lbits | wbase | lparent | lgid (| lmin when it cannot share wbase's words)
static inline size_t ccl_local_lds(const ccl_geom& G, size_t& cap, const ccl_tuning& T)
{
    const size_t nwmax = (size_t)G.rows * G.ww;
    // Foreground: room for one segment per word of the strip (a full mask) + 2, the size of the wbase array whose LDS lmin then
    // reuses; denser strips (speckle) take the global fallback.  Background pass of the contour code: every empty word is a
    // segment and every foreground edge adds one, so it gets its own lmin array and 1024 more entries.
    cap = G.invert ? nwmax + 1024 : nwmax + 2;
    if (T.cl_cap >= 64 && T.cl_cap < cap) cap = T.cl_cap;
    size_t lds_local = nwmax * 8 + (nwmax + 2) * 4 + (cap <= nwmax + 2 ? 2 : 3) * cap * 4;
    if (lds_local > 64 * 1024 && G.invert) { cap = nwmax + 2; lds_local = nwmax * 8 + (nwmax + 2) * 4 + 2 * cap * 4; }
    return lds_local;
}

static inline c3_plan c3_make_plan(const ccl_geom& G, u32 max_ids)
{
    c3_plan P = {0, 0, 0, 0};
    for (int R = 32; R >= 2; R >>= 1) {
        const u32 ids = (u32)R * (u32)G.wb;
        if (ids <= max_ids && (ids % 32u) == 0 && R * G.ww <= 512) { P.R = R; P.ids = ids; break; }
    }
    if (!P.R || G.ww > 64) return P;
    P.strips = (G.h + P.R - 1) / P.R;
    P.ok = P.strips <= C3_MAX_STRIPS ? 1 : 0;
    return P;
}

static inline size_t c3_link_lds(const ccl_geom& G, const c3_plan& P) { return (size_t)P.R * G.ww * 8 + (size_t)P.ids * 4 + (size_t)P.ids / 32 * 4; }
static inline size_t c3_label_lds(const ccl_geom& G, const c3_plan& P, size_t nrcap, size_t accn)
{
    const size_t nrmax = nrcap ? nrcap : (size_t)P.ids / 2;
    return (size_t)P.R * G.ww * 8 + nrmax * 4 + (size_t)P.ids * 2 + nrmax * 2 + (size_t)P.ids / 32 * 4 * 5 + 8 + accn * 4 * 5;
}

// Everything vpk_ccl decides before its first launch.  The fields after `two_level` are zero unless it is set; P3.ok says "the
// geometry suits the crowded-frame kernels" - the dispatcher still clears it when the device refuses their dynamic LDS.
struct ccl_plan {
    ccl_geom G;
    int strips;                        // of the strip-local pass, G.rows each
    u32 gpr, magic;                    // label-write kernels: 4-px groups per row and the multiplier that divides by it
    size_t cap2, rc, tail_words, lds2; // k_ccl2_local: union-find entries, components with LDS accumulators, words of its tail, dynamic LDS
    bool two_level;
    int mcap;                          // components per frame k_ccl2_merge accepts
    c3_plan P3;
    bool c3_tall;                      // strips of more than 8192 ids: twice the threads per block (one word per thread still)
    size_t lds3a, lds3b, lds3c;        // dynamic LDS of k_ccl3_link, of the heavy and of the light k_ccl3_label
};

static inline ccl_plan ccl_make_plan(int w, int h, int numbering, int ccl_levels, int ccl_mcap, const ccl_tuning& T)
{
    ccl_plan P = {};
    ccl_geom& G = P.G;
    ccl_make_geom(G, w, h, numbering, 0, 0, T);
    const int strips = P.strips = (h + G.rows - 1) / G.rows;
    const u32 gpr = P.gpr = (u32)((w + 3) / 4);
    P.magic = (u32)((0x100000000ull + gpr - 1) / gpr);

    const size_t nwmax = (size_t)G.rows * G.ww;
    const size_t cap2 = P.cap2 = nwmax + 2;
    const size_t rc = P.rc = 96;   // components per strip with LDS accumulators (44 B each)
    size_t tail_words = std::max(rc * 11, cap2);    // union queue, then root -> list place (cap words), then the accumulators
    tail_words += tail_words & 1;
    P.tail_words = tail_words;
    const size_t list_words = nwmax + (nwmax + 1) / 2 + ((nwmax + (nwmax + 1) / 2) & 1);   // wbase + word list, padded to 8 bytes
    const size_t lds2 = P.lds2 = nwmax * 8 + (list_words + cap2 + tail_words) * 4;         // 1080p: 21.8 KB, seven blocks per CU
    P.two_level = ccl_levels == 2 && lds2 <= 64 * 1024 && G.ww <= 64 && G.rows <= CL_ROWS && strips <= C2_MAXSTRIPS &&
                  (G.rows % WR_ROWS) == 0 && (G.rows % 8) == 0 && (size_t)strips <= c2_strips_max(h);
    if (!P.two_level) return P;
    P.mcap = (ccl_mcap >= 0 && ccl_mcap < C2_MCAP) ? ccl_mcap : C2_MCAP;
    // frames the merge hands over go to the crowded-frame kernels of vp_ccl3.inl when the geometry suits them (it does for every
    // frame up to 8192 px wide), otherwise to the one-level kernels
    c3_plan& P3 = P.P3;
    P3 = c3_make_plan(G, std::min<u32>(T.c3_ids, C3_IDS));
    P.c3_tall = P3.ids > 8192;
    if (P3.ok && !T.c3_off && (size_t)P3.strips + 1 <= c3_strips_cap(h)) {
        P.lds3a = c3_link_lds(G, P3);
        P.lds3b = c3_label_lds(G, P3, 0, C3_ACC);
        P.lds3c = c3_label_lds(G, P3, C3_LIGHT_ROOTS, C3_LIGHT_ACC);
    } else {
        P3.ok = 0;
    }
    return P;
}
