// Host arithmetic of the contour dispatch (vpk_find_contours, vp_contours.inl): what is refused, which form runs, the grid of every
// launch, the rounds of the pointer-jumping sequences, and the workspace - ONE table of (name, bytes) in placement order that both the
// size of the scratch region (vp_contours_ws_bytes, vp_contour_tree_ws_bytes) and its placement in vpk_find_contours read.  Plain C++ - no HIP types, no kernels - so that all
// of it is checked without a GPU (tests/native/contours_plan_main.cpp against tests/golden/contours_plan.txt).  The layout of the
// result header of the single-image entries (vp_api_label.hip) and the choice of the form (VP_CT_MANY) live here as well.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include "../../include/vp.h"

#define CTJ_LDS_HEADS 8192     // heads of a frame whose tables fit the LDS of the one block of k_ct_jump (16 B each)
#define CTM_SEQ 32             // launches form: flag slots per round sequence, so fewer rounds than this
#define CTM_NFLAGS (3 * CTM_SEQ)
#define CT_HOPS 3              // jumps per launch of a round sequence (ctj_args::hops, ctt_args::hops)

// heads a frame can have: 1.25 per pixel, in multiples of 64
static inline size_t ct_hcap(int w, int h) { const size_t npx = (size_t)w * h; return (npx + npx / 4 + 64 + 63) / 64 * 64; }

// sort key of the hierarchy pass = parent + 1 in [0, max_contours], max_contours + 1 past the borders
static inline int ct_key_bits(int max_contours)
{
    int b = 1;
    while (b < 31 && ((unsigned)max_contours + 1u) >> b) b++;
    return b;
}

// a launch of CT_HOPS steps multiplies the shortest window (distance jumped) by CT_HOPS + 1 at least: rounds that always suffice for `len`
static inline int ct_rounds(size_t len)
{
    int rounds = 2;
    for (size_t reach = 1; reach < len; reach *= (size_t)(CT_HOPS + 1)) rounds++;
    return rounds;
}

// VP_CT_MANY=0 / 1: the bookkeeping always in one block per frame / always as launches over the chip; unset (or negative): as launches
// when the last pass counted more heads than the block's LDS tables hold.  Read on every call: the tests switch it between calls.
static inline bool ct_want_many(uint32_t heads_hint, bool* forced = nullptr)
{
    const char* e = getenv("VP_CT_MANY");
    const int v = e ? atoi(e) : -1;
    if (forced) *forced = v >= 0;
    return v >= 0 ? v != 0 : heads_hint > (uint32_t)CTJ_LDS_HEADS;
}

// Result header of a single-image call, one block so that one copy (or the mirror) brings it back:
// info (16 B: n_contours, n_points, heads) | counts[mc] | offsets[mc] | (tree: hierarchy[mc][4]) | is_hole[mc].  Byte offsets.
struct ct_hdr_layout { size_t counts, offsets, hier, is_hole, bytes; };
static inline ct_hdr_layout ct_hdr(int mc, bool tree)
{
    ct_hdr_layout L;
    L.counts = 16;
    L.offsets = L.counts + (size_t)mc * 4;
    L.hier = L.offsets + (size_t)mc * 4;
    L.is_hole = L.hier + (tree ? (size_t)mc * 16 : 0);
    L.bytes = L.is_hole + (size_t)mc;
    return L;
}

// ---- workspace ----------------------------------------------------------------------------------------------------------------
// Order in the scratch region.  Every array starts on a 256-B boundary, so a table costs the sum of ct_align(bytes) (+ slack).
enum { CTW_HMAPS, CTW_HBASE, CTW_CNT8, CTW_HEAD_PIX, CTW_HRANK, CTW_HKEY, CTW_HEXT, CTW_NODE, CTW_NODE2, CTW_STARTS, CTW_SHEAD, CTW_AUX, CTW_PARTSUM,
       CTW_FLAGS, CTW_CSUM, CTW_BASE,
       CTW_TCOUNTS = CTW_BASE, CTW_TOFFSETS, CTW_THOLE, CTW_PAR, CTW_KEY, CTW_VAL, CTW_SKEY, CTW_SVAL, CTW_FC, CTW_NS, CTW_NW, CTW_TOUR, CTW_SORT, CTW_SPARE,
       CTW_ALL };
struct ct_ws_entry { const char* name; size_t bytes; };

static inline size_t ct_align(size_t n) { return (n + 255) / 256 * 256; }   // = vp_align (vp_internal.h)
static inline size_t ct_ws_total(const ct_ws_entry* e, int count, size_t slack)
{
    size_t t = slack;
    for (int i = 0; i < count; i++) t += ct_align(e[i].bytes);
    return t;
}

// e[CTW_HMAPS .. CTW_BASE): n frames of w x h.  sizeof(ct_aux) = 8.
static inline void ct_ws_base(ct_ws_entry* e, int w, int h, int n, int max_contours)
{
    const size_t words = (size_t)n * h * ((w + 63) / 64), hcap = ct_hcap(w, h), heads = hcap * n;
    e[CTW_HMAPS] = {"hmaps", words * 32};
    e[CTW_HBASE] = {"hbase", words * 4};
    e[CTW_CNT8] = {"cnt8", words};
    e[CTW_HEAD_PIX] = {"head_pix", heads * 4};
    e[CTW_HRANK] = {"hrank", heads * 4};
    e[CTW_HKEY] = {"hkey", heads * 4};
    e[CTW_HEXT] = {"hext", heads * 4};
    e[CTW_NODE] = {"node", heads * 8};
    e[CTW_NODE2] = {"node2", heads * 8};
    e[CTW_STARTS] = {"starts", (size_t)n * max_contours * 4};
    e[CTW_SHEAD] = {"shead", (size_t)n * max_contours * 4};
    e[CTW_AUX] = {"aux", (size_t)8 * n};
    e[CTW_PARTSUM] = {"partsum", words / 64 + 4 * (size_t)n};      // >= 4 B per block of 256 words per frame (k_ct_headmaps' grid)
    e[CTW_FLAGS] = {"flags", (size_t)n * CTM_NFLAGS * 4};
    e[CTW_CSUM] = {"csum", (hcap / 1024 + 2) * 4 * n};
}

// e[CTW_TCOUNTS .. CTW_ALL): the hierarchy pass of one image; sort_bytes: what the radix sort asks for (hipcub, queried by the caller)
static inline void ct_ws_tree(ct_ws_entry* e, int max_contours, size_t sort_bytes)
{
    const size_t mc = (size_t)max_contours;
    e[CTW_TCOUNTS] = {"tcounts", mc * 4};
    e[CTW_TOFFSETS] = {"toffsets", mc * 4};
    e[CTW_THOLE] = {"thole", mc};
    e[CTW_PAR] = {"par", mc * 4};
    e[CTW_KEY] = {"key", mc * 4};
    e[CTW_VAL] = {"val", mc * 4};
    e[CTW_SKEY] = {"skey", mc * 4};
    e[CTW_SVAL] = {"sval", mc * 4};
    e[CTW_FC] = {"fc", (mc + 1) * 4};
    e[CTW_NS] = {"ns", mc * 4};
    e[CTW_NW] = {"nw", mc * 4};
    e[CTW_TOUR] = {"tour", (2 * mc + 2) * 8};
    e[CTW_SORT] = {"sort", sort_bytes};
    e[CTW_SPARE] = {"spare", mc * 4};        // no kernel reads it: the reservation has always counted one array more than the pass carves
}

static inline size_t ct_ws_base_bytes(int w, int h, int n, int max_contours)
{
    ct_ws_entry e[CTW_BASE];
    ct_ws_base(e, w, h, n, max_contours);
    return ct_ws_total(e, CTW_BASE, 8192);
}
static inline size_t ct_ws_tree_bytes(int max_contours, size_t sort_bytes)
{
    ct_ws_entry e[CTW_ALL];
    ct_ws_tree(e, max_contours, sort_bytes);
    return ct_ws_total(e + CTW_BASE, CTW_ALL - CTW_BASE, 4096);
}

// ---- the plan -----------------------------------------------------------------------------------------------------------------
// Everything vpk_find_contours decides before its first launch.  status != VP_OK: refused, `why` is the message, the rest means nothing.
struct ct_plan {
    int status;
    const char* why;
    bool tree;                       // the hierarchy pass runs (RETR_CCOMP / RETR_TREE, one image, a buffer for the rows)
    bool mirror;                     // the kernels write the results into the caller's pinned buffers as well (one image)
    bool hint_slots;                 // the prefix kernel leaves the frames' head counts in the context's pinned slots (vp_ct_batch_hint)
    int seg_mode;                    // 0: RETR_EXTERNAL, 1: every border (the hierarchy pass selects from the full list)
    int defer_big;                   // one block, one image: more than CTJ_LDS_HEADS heads are reported, not worked through
    unsigned skip_above;             // ... and the follower passes skip such a frame
    int nwords;                      // 64-pixel words of a frame
    size_t words, hcap;              // words of the batch; heads per frame
    unsigned wgrid, hgrid, mg, sg;   // blocks per frame (grid.x; grid.y = n): per 256 words, over the head list, of k_ctm / of its sums and scans
    int rounds;                      // of each k_ctm round sequence
    int rounds_tree, key_bits;       // tree: rounds of the two jump loops, bits the sort looks at
    unsigned nb, tb, jb, jtb;        // tree: blocks over the borders, over the tour, and of the jump kernels over either (they stride)
    int nws;                         // entries of ws[] in use: CTW_BASE, or CTW_ALL with the hierarchy pass
    ct_ws_entry ws[CTW_ALL];
};

static inline ct_plan ct_make_plan(int w, int h, int n, int mode, int method, int max_contours, bool have_hier, bool have_mirror, bool many_heads,
                                   bool defer_big, uint32_t heads_hint, size_t sort_bytes)
{
    ct_plan P = {};
    auto refuse = [&P](const char* why) { P.status = VP_ERR_INVALID; P.why = why; return P; };
    P.tree = (mode == 2 || mode == 3) && have_hier && n == 1;
    if (mode != 0 && mode != 1 && !P.tree) return refuse("contour mode");
    if (method != 1 && method != 2) return refuse("contour approximation");
    if ((size_t)w * h >= (1u << 29)) return refuse("contours: image too large");
    P.nwords = h * ((w + 63) / 64);
    P.words = (size_t)n * P.nwords;
    P.hcap = ct_hcap(w, h);
    // (cannot happen below 2^29 pixels - 17 rounds; the host test proves it for every admitted size - but k_ctm's flag slots rely on it)
    P.rounds = ct_rounds(P.hcap);
    if (P.rounds >= CTM_SEQ) return refuse("contours: image too large");
    P.mirror = have_mirror && n == 1;
    P.hint_slots = n > 1 || !have_mirror;
    P.seg_mode = mode == 0 ? 0 : 1;
    P.defer_big = (defer_big && n == 1 && !many_heads) ? 1 : 0;
    P.skip_above = P.defer_big ? (unsigned)CTJ_LDS_HEADS : 0u;
    P.wgrid = (unsigned)((P.nwords + 255) / 256);
    // heads per frame are not known on the host: a fixed number of blocks per frame walks the head list (a real mask has a few
    // thousand heads; empty blocks of a grid sized for the worst case would cost more than the work)
    // (one image: the head count of the context's last single-image pass sizes the grid - two items per head, half as much again -
    // instead of a thousand blocks of which thirty find work; the loops stride over the grid, so a wrong guess only costs time)
    size_t hblocks = (size_t)std::max(32, std::min(1024, 8192 / n));
    if (n == 1 && heads_hint) hblocks = std::min<size_t>(hblocks, std::max<size_t>(32, ((size_t)heads_hint * 3 + 255) / 256));
    P.hgrid = (unsigned)std::min<size_t>((P.hcap + 255) / 256, hblocks);
    P.mg = (unsigned)std::max(32, std::min(1024, 8192 / n));
    P.sg = (unsigned)std::max(8, std::min(256, 2048 / n));
    ct_ws_base(P.ws, w, h, n, max_contours);
    P.nws = CTW_BASE;
    if (P.tree) {
        P.rounds_tree = ct_rounds(2 * (size_t)max_contours + 2);
        P.key_bits = ct_key_bits(max_contours);
        P.nb = (unsigned)((max_contours + 256) / 256);
        P.tb = (unsigned)((2 * (size_t)max_contours + 2 + 255) / 256);
        P.jb = std::min(P.nb, 1024u);
        P.jtb = std::min(P.tb, 1024u);
        ct_ws_tree(P.ws, max_contours, sort_bytes);
        P.nws = CTW_ALL;
    }
    return P;
}
