// Host arithmetic of the bit-plane morphology (vp_morph.hip, planned in vp_api_morph_chain.hip): how a rect erode / dilate / OPEN /
// CLOSE becomes stages of extents <= 31, which kernel a stage plan goes to (one of the specialised instantiations with 64- or 32-row
// strips, or the runtime-plan kernel) with its LDS bytes, and how a stage list is grouped into launches with the bit plane every
// launch reads and writes.  Plain C++ - no HIP types, no kernels - and a pure function of its arguments, like vp_ccl_plan.h and
// vp_dist_plan.h; tests/native/morph_plan_main.cpp enumerates it on the host.
#pragma once
#include <stddef.h>
#include <vector>

struct vp_bitstage { int dilate; int l, r, u, d; };  // window [-l, r] x [-u, d]
#define VP_MAX_STAGES 32
struct vp_bitplan { int n; vp_bitstage s[VP_MAX_STAGES]; };
// words per row of a bit image
static inline int vp_ww(int w) { return (w + 63) / 64; }

#define MB_THREADS 512
#define MB_STRIP 32                          // output rows per block: every kernel's default
#define MB_TALL_STRIP 64                     // ... of the specialised kernels when the strip fits MB_TALL_LDS
#define MB_MAX_EXTENT 31                     // the funnel shifts take 1..31
#define MB_TALL_LDS ((size_t)40 * 1024)      // four blocks per CU
#define MB_SYM_LDS ((size_t)64 * 1024)       // the specialised kernels stay below the opt-in
#define MB_PLAN_LDS ((size_t)160 * 1024)     // the runtime-plan kernel's ceiling (opt-in above 64 KB)
#define MB_GROUP_LDS ((size_t)150 * 1024)    // what the grouping fills of it
static_assert(MB_GROUP_LDS <= MB_PLAN_LDS, "bit morphology: a grouped launch above the runtime-plan kernel's ceiling");

// operation codes: those of include/vp.h (vp_api_morph_chain.hip asserts that they agree)
enum { MB_OP_ERODE = 0, MB_OP_DILATE = 1, MB_OP_OPEN = 2, MB_OP_CLOSE = 3 };

// ---- stages ---------------------------------------------------------------------------------------------------------

struct mb_rect { int kw, kh, ax, ay; };

// Adds one rect erode/dilate to a stage list, split so that every stage has extents <= 31 (the kernels' funnel shifts).
static inline void mb_push_rect_stage(std::vector<vp_bitstage>& v, int dilate, const mb_rect& k)
{
    int l = k.ax, r = k.kw - 1 - k.ax, u = k.ay, d = k.kh - 1 - k.ay;
    // merge with the previous stage of the same kind (erode∘erode / dilate∘dilate with cv2's border
    // rule equal one pass with summed extents: the image is a box, clamping an intermediate sample
    // into it never increases a coordinate distance)
    if (!v.empty() && v.back().dilate == dilate) {
        l += v.back().l; r += v.back().r; u += v.back().u; d += v.back().d;
        v.pop_back();
    }
    do {
        vp_bitstage s;
        s.dilate = dilate;
        s.l = l > MB_MAX_EXTENT ? MB_MAX_EXTENT : l; s.r = r > MB_MAX_EXTENT ? MB_MAX_EXTENT : r;
        s.u = u > MB_MAX_EXTENT ? MB_MAX_EXTENT : u; s.d = d > MB_MAX_EXTENT ? MB_MAX_EXTENT : d;
        l -= s.l; r -= s.r; u -= s.u; d -= s.d;
        v.push_back(s);
    } while (l | r | u | d);
}

// false: not one of the four operations
static inline bool mb_stages_for_op(std::vector<vp_bitstage>& v, int op, const mb_rect& k)
{
    switch (op) {
        case MB_OP_ERODE: mb_push_rect_stage(v, 0, k); break;
        case MB_OP_DILATE: mb_push_rect_stage(v, 1, k); break;
        case MB_OP_OPEN: mb_push_rect_stage(v, 0, k); mb_push_rect_stage(v, 1, k); break;
        case MB_OP_CLOSE: mb_push_rect_stage(v, 1, k); mb_push_rect_stage(v, 0, k); break;
        default: return false;
    }
    return true;
}

static inline bool mb_stage_ok(const vp_bitstage& s)
{
    return s.l >= 0 && s.l <= MB_MAX_EXTENT && s.r >= 0 && s.r <= MB_MAX_EXTENT && s.u >= 0 && s.d >= 0;
}

// ---- which kernel a plan goes to ---------------------------------------------------------------------------------------

// The specialised shapes (square kernels, centre anchor): X(stages, radius 0, radius 1, radius 2, kinds), bit k of kinds = stage k
// dilates.  vp_morph.hip instantiates k_morph_bits_sym from this list and mb_sym_lookup searches it: one list, typed once.
#define MB_SYM_SHAPES(X) \
    X(3, 2, 4, 2, 2)  /* OPEN 5x5 + CLOSE 5x5  (erode, dilate x2 merged, erode)      - modules/red_buoy.py:31-33 */ \
    X(3, 2, 4, 2, 5)  /* CLOSE 5x5 + OPEN 5x5 */ \
    X(2, 2, 2, 0, 2)  /* OPEN 5x5                                                   - modules/bins.py:23-24 */ \
    X(2, 2, 2, 0, 1)  /* CLOSE 5x5 */ \
    X(3, 1, 2, 1, 2)  /* OPEN 3x3 + CLOSE 3x3 */ \
    X(3, 1, 2, 1, 5)  /* CLOSE 3x3 + OPEN 3x3 */ \
    X(2, 1, 1, 0, 2)  /* OPEN 3x3 */ \
    X(2, 1, 1, 0, 1)  /* CLOSE 3x3 */ \
    X(1, 1, 0, 0, 0) X(1, 1, 0, 0, 1)   /* erode / dilate 3x3 */ \
    X(1, 2, 0, 0, 0) X(1, 2, 0, 0, 1)   /* erode / dilate 5x5 */

struct mb_sym_shape { int ns, r[3], kind; };
#define MB_SYM_ROW(NS, A, B, C, K) {NS, {A, B, C}, K},
static const mb_sym_shape mb_sym_shapes[] = {MB_SYM_SHAPES(MB_SYM_ROW)};
#undef MB_SYM_ROW
#define MB_SYM_COUNT ((int)(sizeof(mb_sym_shapes) / sizeof(mb_sym_shapes[0])))

static inline int mb_sym_halo(const mb_sym_shape& s) { return s.r[0] + (s.ns > 1 ? s.r[1] : 0) + (s.ns > 2 ? s.r[2] : 0); }

// index into mb_sym_shapes, or -1 when the plan is not one of the specialised shapes
static inline int mb_sym_lookup(const vp_bitplan& plan)
{
    if (plan.n < 1 || plan.n > 3) return -1;
    int rad[3] = {0, 0, 0}, kind = 0;
    for (int i = 0; i < plan.n; i++) {
        const vp_bitstage& s = plan.s[i];
        if (s.l != s.r || s.l != s.u || s.l != s.d) return -1;
        rad[i] = s.l;
        kind |= (s.dilate ? 1 : 0) << i;
    }
    for (int k = 0; k < MB_SYM_COUNT; k++) {
        const mb_sym_shape& q = mb_sym_shapes[k];
        if (plan.n == q.ns && rad[0] == q.r[0] && rad[1] == q.r[1] && rad[2] == q.r[2] && kind == q.kind) return k;
    }
    return -1;
}

// LDS of a specialised kernel: two buffers of (strip + 2 halo) rows
static inline size_t mb_sym_lds(int strip, int halo, int ww) { return (size_t)2 * (strip + 2 * halo) * ww * 8; }
// 64-row strips when they fit 40 KB of LDS (four blocks per CU; 1080p: 38 KB): the halo rows every stage recomputes are then 20 % of the
// strip instead of 33 % (74 instead of 78 us per 128 frames); wider frames keep 32 rows
static inline int mb_sym_strip(int halo, int w, int h, bool tall_ok)
{
    return (tall_ok && h > MB_TALL_STRIP && mb_sym_lds(MB_TALL_STRIP, halo, vp_ww(w)) <= MB_TALL_LDS) ? MB_TALL_STRIP : MB_STRIP;
}
// LDS of the runtime-plan kernel: two buffers of 32 rows and the vertical extents of every stage
static inline size_t mb_plan_lds(const vp_bitplan& plan, int ww)
{
    int halo = 0;
    for (int i = 0; i < plan.n; i++) halo += plan.s[i].u + plan.s[i].d;
    return (size_t)2 * (MB_STRIP + halo) * ww * 8;
}

// what vpk_morph_bits launches for one plan.  sym: index into mb_sym_shapes or -1 (the runtime-plan kernel); ok = 0: no kernel takes
// it (the caller splits the plan)
struct mb_kernel { int ok, sym, strip; size_t lds; };
static inline mb_kernel mb_choose_kernel(const vp_bitplan& plan, int w, int h, bool sym_ok, bool tall_ok)
{
    mb_kernel K;
    const int ww = vp_ww(w);
    K.sym = sym_ok ? mb_sym_lookup(plan) : -1;
    if (K.sym >= 0) {
        const int halo = mb_sym_halo(mb_sym_shapes[K.sym]);
        K.strip = mb_sym_strip(halo, w, h, tall_ok);
        K.lds = mb_sym_lds(K.strip, halo, ww);
        K.ok = K.lds <= MB_SYM_LDS;
        if (K.ok) return K;
    }
    K.sym = -1;
    K.strip = MB_STRIP;
    K.lds = mb_plan_lds(plan, ww);
    K.ok = K.lds <= MB_PLAN_LDS;
    return K;
}

// ---- launches ----------------------------------------------------------------------------------------------------------------

// The bit planes of a run: the caller's input, which no launch writes; two scratch planes; and the output, which the last launch and
// only it writes (bits and / or the 0/255 mask).  The last launch never reads the second scratch plane, so a caller may back that
// one with the memory of its output plane.
enum { MB_BUF_IN = 0, MB_BUF_SCRATCH = 1, MB_BUF_SCRATCH2 = 2, MB_BUF_OUT = 3 };
struct mb_launch { int first, count; int src, dst; };   // stages [first, first + count) of the list

// Groups a stage list into launches whose halo fits MB_GROUP_LDS of the runtime-plan kernel.  false: even the first stage alone does
// not fit (the image is too wide for the strip).
static inline bool mb_group_stages(const std::vector<vp_bitstage>& st, int ww, std::vector<mb_launch>& out)
{
    out.clear();
    size_t i = 0;
    while (i < st.size()) {
        mb_launch L;
        L.first = (int)i; L.count = 0; L.src = L.dst = -1;
        int halo = 0;
        while (i < st.size() && L.count < VP_MAX_STAGES) {
            const int nh = halo + st[i].u + st[i].d;
            const size_t lds = (size_t)2 * (MB_STRIP + nh) * ww * 8;
            if (L.count > 0 && lds > MB_GROUP_LDS) break;
            if (L.count == 0 && lds > MB_GROUP_LDS) { out.clear(); return false; }
            L.count++; i++;
            halo = nh;
        }
        out.push_back(L);
    }
    // the last launch writes the output, the one before it the first scratch plane, and the earlier ones alternate backwards from
    // there: no launch reads what it writes, and the input plane is only ever read
    const size_t n = out.size();
    for (size_t k = 0; k < n; k++) {
        out[k].dst = k + 1 == n ? MB_BUF_OUT : (((n - 2 - k) & 1) ? MB_BUF_SCRATCH2 : MB_BUF_SCRATCH);
        out[k].src = k == 0 ? MB_BUF_IN : out[k - 1].dst;
    }
    return true;
}
