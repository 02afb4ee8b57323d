// 8-connected component labelling with statistics on bit-packed masks, for gfx950.
//
// North-star replacement for the cv2.findContours stage of utils/feature.py:5-40 /
// modules/red_buoy.py:38: output equals cv2.connectedComponentsWithStats(mask, 8, CV_32S)
// (labels, stats rows [left, top, width, height, area], centroids; row 0 = background).
//
// The union-find runs on *word segments* — maximal runs of 1-bits inside one 64-bit word of a
// row — not on pixels.  A segment's id encodes where it starts, in an order that matches cv2's
// numbering: for VP_CCL_BLOCK2X2, id = 2*((y/2)*Wb + x/2) + (y&1), i.e. the raster index of the
// aligned 2x2 block holding the segment's first pixel.  Linking always points the larger id at
// the smaller, so a component's root is its smallest id and cv2's label for the component is
// simply the rank of that root among all roots.  Ranks come from a bitmap of roots + popcount
// prefix — no sort.  The label image (4 B/px, the dominant HBM traffic of the whole chain) is
// written exactly once, by a streaming kernel.
//
//   k_ccl_local    per 32-row strip, in LDS: segments -> compact ids -> union-find (across word boundaries in a
//                  row and with the row above, 8-conn) -> parent[id] = smallest id of the strip-local component;
//                  clears the strip's slice of the root bitmap and marks the strip-local representatives
//   k_ccl_boundary unions between the first row of a strip and the row above it (global CAS union-find);
//                  a root that gets linked loses its bit in the bitmap, so the bitmap ends up = exact roots
//   (k_ccl_init + k_ccl_link: the same in global memory only, fallback for very wide images)
//   k_ccl_rank     per frame: exclusive popcount prefix over the bitmap, nlabels, zero accumulators; extra blocks
//                  of the same launch reduce the background row (label 0) without atomics
//   k_ccl_stats    label = rank(root)+1 per segment -> seglabel[id], wordlabel[word]; per-block LDS aggregation,
//                  then one set of global atomics per (block, label)
//   k_ccl_final    accumulators -> stats (i32 x5) + centroids (f64 x2)
//   k_ccl_write    bits + wordlabel (+ seglabel for words holding several segments) -> int32 label image
//
// Measured and dropped (git history has them; DESIGN.md section 5 lists the numbers): one 1024-thread block per frame running
// boundary -> rank -> stats -> final with block barriers; writing the stats rows from the last block of k_ccl_stats; 2-4 internal
// streams; 64-row strips; a per-strip rank fed by root counters; path compression after the boundary unions; replicated
// accumulators; label write of one half of the batch under the bookkeeping of the other.
#include "vp_internal.h"
#include "vp_ccl_dev.h"
#include "vp_ccl_hint.h"
#include <limits.h>
#include <cstdio>
#include <string.h>
#include <cstdlib>
#include <algorithm>
#include <vector>
#include <hipcub/device/device_radix_sort.hpp>     // (vp_contours.inl: the children of each border in scan order, RETR_CCOMP / RETR_TREE)

struct ccl_acc {   // 48 B
    u32 area;
    int minx, miny, maxx, maxy;
    u32 pad;
    u64 sx, sy;
};

struct contrib { u32 area; int minx, maxx, miny, maxy; u32 pad; u64 sx, sy; };

// every entry "empty": what acc_commit expects to add to
__global__ __launch_bounds__(256) void k_ccl3_acc_init(ccl_acc* __restrict__ acc, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        ccl_acc z;
        z.area = 0; z.minx = INT_MAX; z.miny = INT_MAX; z.maxx = INT_MIN; z.maxy = INT_MIN; z.pad = 0; z.sx = 0; z.sy = 0;
        acc[i] = z;
    }
}

#define RK_PARTS 8
#define BG_PARTS 8
#define C2_RC 128              // two-level labelling (vp_ccl2.inl): stride of the per-strip component tables
struct c2_box { int minx, maxx, miny, maxy; };

size_t vp_ccl_nids(int w, int h)
{
    return ccl_nids(w, h);
}

// which of the two labelling launches takes a strip (vp_ccl3.inl): one byte per (frame, strip)
static size_t c3_items_bytes(int n, int h) { return (size_t)n * c3_strips_cap(h); }

void vp_ccl_ws_want(vp_ws_frame& W, int w, int h, int n, int max_labels, vp_ccl_ws* out)
{
    const size_t nids = vp_ccl_nids(w, h);
    W.want(&out->parent, nids * 4 * n);
    W.want(&out->seglabel, nids * 4 * n);
    W.want(&out->flags, nids / 8 * n);
    W.want(&out->prefix, nids / 8 * n);
    W.want(&out->acc, sizeof(ccl_acc) * (size_t)max_labels * n);
    W.want(&out->wordlabel, (size_t)n * h * vp_ww(w) * 4);
    W.want(&out->bgpart, sizeof(contrib) * BG_PARTS * (size_t)n);
    const size_t ns = c2_strips_max(h) * (size_t)n;
    W.want(&out->c2_ncomp, ns * 4);
    W.want(&out->c2_recs, ns * C2_RC * sizeof(contrib));
    W.want(&out->c2_bgbox, ns * sizeof(c2_box));
    W.want(&out->c2_label, ns * C2_RC * 4);
    W.want(&out->c2_crowded, (size_t)n * 4);
    W.want(&out->c3_child, nids / 8 * n);
    W.want(&out->c3_lroot, nids / 8 * n);
    W.want(&out->c3_clist, (size_t)n * 4);
    W.want(&out->c3_ncrowded, 4);
    W.want(&out->c3_state, (size_t)n * C3_STATE_BYTES);
    W.want(&out->c3_tot, (size_t)n * c3_strips_cap(h) * 40);              // sizeof(contrib)
    W.want(&out->c3_barr, (size_t)n * c3_strips_cap(h) * 12);   // per frame: boundary arrivals | boundaries done per strip | roots per strip
    W.want(&out->c3_items, c3_items_bytes(n, h));     // per (handed-over frame, strip): 1 = light labelling launch, 2 = heavy
}

// ---- whole-image global-memory path (fallback for images too wide for the LDS strip kernel) ---------------
// The bodies of the one-level kernels are device functions of (block index, frame): the kernels below call them with their own
// blockIdx, k_ccl2_finish (vp_ccl2.inl) walks the block indices of one frame in a single block.
// grid: (ceil(h*ww/256), n); flags zeroed by a memset before k_ccl_init
__device__ __forceinline__ void ccl_init_body(const u64* __restrict__ bits, const ccl_geom& G, u32* parent, u32* flags, int vbx, int frame)
{
    const int idx = vbx * 256 + threadIdx.x;
    if (idx >= G.h * G.ww) return;
    const int y = idx / G.ww, j = idx - y * G.ww;
    const u64 w = ccl_word(G, bits + (size_t)frame * G.h * G.ww, idx, j);
    if (!w) return;
    u32* p = parent + (size_t)frame * G.nids;
    u32* f = flags + (size_t)frame * G.nw32;
    u64 starts = w & ~(w << 1);
    while (starts) {
        const int s = __ffsll((long long)starts) - 1;
        starts &= starts - 1;
        const u32 id = seg_id(G, y, 64 * j + s);
        p[id] = id;
        atomicOr(f + (id >> 5), 1u << (id & 31));
    }
}
__global__ __launch_bounds__(256) void k_ccl_init(const u64* __restrict__ bits, ccl_geom G, u32* __restrict__ parent, u32* __restrict__ flags)
{
    ccl_init_body(bits, G, parent, flags, (int)blockIdx.x, (int)blockIdx.y);
}

__device__ __forceinline__ void ccl_link_body(const u64* __restrict__ bits, const ccl_geom& G, u32* parent, u32* flags, int vbx, int frame)
{
    const int idx = vbx * 256 + threadIdx.x;
    if (idx >= G.h * G.ww) return;
    const u64* fb = bits + (size_t)frame * G.h * G.ww;
    const int y = idx / G.ww, j = idx - y * G.ww;
    const u64 w = ccl_word(G, fb, idx, j);
    if (!w) return;
    global_link_word(fb, G, parent + (size_t)frame * G.nids, flags + (size_t)frame * G.nw32, y, j, idx, w, true, true);
}
__global__ __launch_bounds__(256) void k_ccl_link(const u64* __restrict__ bits, ccl_geom G, u32* __restrict__ parent, u32* __restrict__ flags)
{
    ccl_link_body(bits, G, parent, flags, (int)blockIdx.x, (int)blockIdx.y);
}

// One block per (frame, strip of CL_ROWS rows).
// dynamic LDS: lbits[nw] u64 | wbase[nw + 2] u32 | lparent[cap] | lgid[cap] | lmin[cap] (cap <= nw + 2: lmin reuses wbase)
__global__ __launch_bounds__(256) void k_ccl_local(const u64* __restrict__ bits, ccl_geom G, u32* __restrict__ parent,
                                                   u32* __restrict__ flags, int strips, int cap, const u32* __restrict__ only,
                                                   u32* __restrict__ zero_too)   // nullable: bitmap with the layout of `flags`, cleared here
{
    extern __shared__ __attribute__((aligned(16))) u64 cl_lds[];
    __shared__ u32 wsum[4];
    __shared__ u32 total_s;
    const int ww = G.ww;
    const int frame = blockIdx.x / strips, strip = blockIdx.x - frame * strips;
    if (only && !only[frame]) return;   // fallback launch of the two-level path: this frame was resolved there
    const int y0 = strip * G.rows;
    const int nrows = min(G.rows, G.h - y0);
    const int nwmax = G.rows * ww;
    u64* lbits = cl_lds;
    u32* wbase = reinterpret_cast<u32*>(cl_lds + nwmax);
    u32* lparent = wbase + (nwmax + 2);
    const u64* fb = bits + (size_t)frame * G.h * ww;
    CL_FOR_WORDS(r, j, i) lbits[i] = ccl_word(G, fb, (y0 + r) * ww + j, j);
    __syncthreads();
    ccl_local_strip(G, lbits, wbase, lparent, lparent + cap, cap <= nwmax + 2 ? wbase : lparent + 2 * cap, wsum, &total_s, y0, nrows, strip, strips, fb,
                    parent + (size_t)frame * G.nids, flags + (size_t)frame * G.nw32, (u32)cap, zero_too ? zero_too + (size_t)frame * G.nw32 : nullptr);
}

// vertical unions across strip boundaries: grid (strips - 1, n), block = 64 threads over the words of the row
__global__ __launch_bounds__(64) void k_ccl_boundary(const u64* __restrict__ bits, ccl_geom G, u32* __restrict__ parent, u32* __restrict__ flags,
                                                     const u32* __restrict__ only)
{
    if (only && !only[blockIdx.y]) return;
    const int y = (blockIdx.x + 1) * G.rows;
    const u64* fb = bits + (size_t)blockIdx.y * G.h * G.ww;
    u32* p = parent + (size_t)blockIdx.y * G.nids;
    u32* f = flags + (size_t)blockIdx.y * G.nw32;
    for (int j = threadIdx.x; j < G.ww; j += 64) {
        const int idx = y * G.ww + j;
        const u64 w = ccl_word(G, fb, idx, j);
        if (w) global_link_word(fb, G, p, f, y, j, idx, w, false, true);
    }
}

// ---- ranks + background -----------------------------------------------------------------------------------

__device__ __forceinline__ u32 sum_bitpos(u64 z)  // sum of the positions of the set bits
{
    return (u32)__popcll(z & 0xAAAAAAAAAAAAAAAAull) + ((u32)__popcll(z & 0xCCCCCCCCCCCCCCCCull) << 1) +
           ((u32)__popcll(z & 0xF0F0F0F0F0F0F0F0ull) << 2) + ((u32)__popcll(z & 0xFF00FF00FF00FF00ull) << 3) +
           ((u32)__popcll(z & 0xFFFF0000FFFF0000ull) << 4) + ((u32)__popcll(z & 0xFFFFFFFF00000000ull) << 5);
}

__device__ __forceinline__ void contrib_zero(contrib& c)
{
    c.area = 0; c.sx = 0; c.sy = 0; c.minx = INT_MAX; c.maxx = INT_MIN; c.miny = INT_MAX; c.maxy = INT_MIN; c.pad = 0;
}
__device__ __forceinline__ void contrib_merge(contrib& c, const contrib& o)
{
    c.area += o.area; c.sx += o.sx; c.sy += o.sy;
    c.minx = min(c.minx, o.minx); c.maxx = max(c.maxx, o.maxx); c.miny = min(c.miny, o.miny); c.maxy = max(c.maxy, o.maxy);
}
__device__ __forceinline__ void wave_combine(contrib& c)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        c.area += __shfl_xor(c.area, d);
        c.sx += __shfl_xor(c.sx, d);
        c.sy += __shfl_xor(c.sy, d);
        c.minx = min(c.minx, __shfl_xor(c.minx, d));
        c.maxx = max(c.maxx, __shfl_xor(c.maxx, d));
        c.miny = min(c.miny, __shfl_xor(c.miny, d));
        c.maxy = max(c.maxy, __shfl_xor(c.maxy, d));
    }
}

// grid (RK_PARTS + BG_PARTS, n), 256 threads.
// blocks [0, RK_PARTS): exclusive popcount prefix over the root bitmap of one frame — part p first counts the bits
//   of parts < p (the bitmap is 130 KB per 1080p frame, L2-resident), then scans its own slice; the last part also
//   publishes nlabels and zeroes the accumulators.
// blocks [RK_PARTS, RK_PARTS + BG_PARTS): background pixels of a slice of the frame reduced to one record.
__device__ __forceinline__ void ccl_rank_body(const ccl_geom& G, const u32* __restrict__ flags, u32* __restrict__ prefix,
                                              int32_t* __restrict__ nlabels, ccl_acc* __restrict__ acc, int max_labels,
                                              const u64* __restrict__ bits, contrib* __restrict__ bgpart, int vbx, int frame)
{
    __shared__ u32 wsum[4];
    __shared__ u32 wsum2[4];
    __shared__ u32 bcast;
    __shared__ contrib part[4];
    const int f = frame, tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    if (vbx >= RK_PARTS) {
        const int bp = vbx - RK_PARTS;
        const int rper = (G.h + BG_PARTS - 1) / BG_PARTS;
        const int r0 = bp * rper, r1 = min(r0 + rper, G.h);
        const u64* fb = bits + (size_t)f * G.h * G.ww;
        const u64 lastmask = (G.w & 63) ? ((1ull << (G.w & 63)) - 1ull) : ~0ull;
        contrib c;
        contrib_zero(c);
        for (int y = r0 + (tid >> 5); y < r1; y += 8)
            for (int j = tid & 31; j < G.ww; j += 32) {
                u64 z = ~fb[(size_t)y * G.ww + j];
                if (j == G.ww - 1) z &= lastmask;
                if (!z) continue;
                const u32 cnt = (u32)__popcll(z);
                c.area += cnt;
                c.sx += (u64)cnt * (u64)(64 * j) + sum_bitpos(z);
                c.sy += (u64)cnt * (u64)y;
                c.minx = min(c.minx, 64 * j + (__ffsll((long long)z) - 1));
                c.maxx = max(c.maxx, 64 * j + 63 - __clzll(z));
                c.miny = min(c.miny, y);
                c.maxy = max(c.maxy, y);
            }
        wave_combine(c);
        if (lane == 0) part[wv] = c;
        __syncthreads();
        if (tid == 0) {
            for (int k = 1; k < 4; k++) contrib_merge(c, part[k]);
            bgpart[(size_t)f * BG_PARTS + bp] = c;
        }
        return;
    }
    const int partno = vbx;
    const u32 nq = G.nw32 / 4;                               // uint4 words per frame
    const u32 qper = (nq + RK_PARTS - 1) / RK_PARTS;
    const u32 q0 = min((u32)partno * qper, nq), q1 = min(q0 + qper, nq);
    const uint4* fl = reinterpret_cast<const uint4*>(flags + (size_t)f * G.nw32);
    uint4* pf = reinterpret_cast<uint4*>(prefix + (size_t)f * G.nw32);
    // own slice: thread = contiguous run of uint4s, loaded once and kept in registers (RK_OWN covers 1080p..4K)
    constexpr int RK_OWN = 16;
    const u32 per = (q1 - q0 + 255) / 256;
    const u32 lo = min(q0 + (u32)tid * per, q1), hi = min(lo + per, q1);
    uint4 own[RK_OWN];
    u32 cnt = 0;
#pragma unroll
    for (int k = 0; k < RK_OWN; k++) {
        own[k] = make_uint4(0, 0, 0, 0);
        if (lo + k < hi) own[k] = fl[lo + k];
    }
    // bits before this part: independent loads, issued in batches
    u32 before = 0;
#pragma unroll 8
    for (u32 q = tid; q < q0; q += 256) { const uint4 v = fl[q]; before += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w); }
#pragma unroll
    for (int k = 0; k < RK_OWN; k++) cnt += __popc(own[k].x) + __popc(own[k].y) + __popc(own[k].z) + __popc(own[k].w);
    for (u32 q = lo + RK_OWN; q < hi; q++) { const uint4 v = fl[q]; cnt += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w); }   // slices beyond RK_OWN (huge images)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) before += __shfl_xor(before, d);
    u32 inc = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const u32 t = __shfl_up(inc, d); if (lane >= d) inc += t; }
    if (lane == 0) wsum[wv] = before;
    if (lane == 63) wsum2[wv] = inc;
    __syncthreads();
    const u32 base = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    u32 woff = 0;
    for (int k = 0; k < wv; k++) woff += wsum2[k];
    u32 run = base + woff + inc - cnt;
#pragma unroll
    for (int k = 0; k < RK_OWN; k++) {
        if (lo + k < hi) {
            const uint4 v = own[k];
            uint4 o;
            o.x = run; run += __popc(v.x);
            o.y = run; run += __popc(v.y);
            o.z = run; run += __popc(v.z);
            o.w = run; run += __popc(v.w);
            pf[lo + k] = o;
        }
    }
    for (u32 q = lo + RK_OWN; q < hi; q++) {
        const uint4 v = fl[q];
        uint4 o;
        o.x = run; run += __popc(v.x);
        o.y = run; run += __popc(v.y);
        o.z = run; run += __popc(v.z);
        o.w = run; run += __popc(v.w);
        pf[q] = o;
    }
    if (partno == RK_PARTS - 1) {
        if (tid == 255) bcast = run;   // last thread's running count = all bits of the frame
        __syncthreads();
        const int nl = (int)bcast + 1;
        if (tid == 0 && nlabels) nlabels[f] = nl;
        ccl_acc* a = acc + (size_t)f * max_labels;
        const int nz = min(nl, max_labels);
        for (int i = tid; i < nz; i += 256) {
            ccl_acc z;
            z.area = 0; z.minx = INT_MAX; z.miny = INT_MAX; z.maxx = INT_MIN; z.maxy = INT_MIN; z.pad = 0; z.sx = 0; z.sy = 0;
            a[i] = z;
        }
    }
}
__global__ __launch_bounds__(256) void k_ccl_rank(ccl_geom G, const u32* __restrict__ flags, u32* __restrict__ prefix,
                                                  int32_t* __restrict__ nlabels, ccl_acc* __restrict__ acc, int max_labels,
                                                  const u64* __restrict__ bits, contrib* __restrict__ bgpart, const u32* __restrict__ only)
{
    if (only && !only[blockIdx.y]) return;
    ccl_rank_body(G, flags, prefix, nlabels, acc, max_labels, bits, bgpart, (int)blockIdx.x, (int)blockIdx.y);
}

// ---- per-label statistics ----------------------------------------------------------------------------------

__device__ __forceinline__ void acc_commit(ccl_acc* a, const contrib& c)
{
    atomicAdd(&a->area, c.area);
    atomicAdd((unsigned long long*)&a->sx, (unsigned long long)c.sx);
    atomicAdd((unsigned long long*)&a->sy, (unsigned long long)c.sy);
    atomicMin(&a->minx, c.minx);
    atomicMax(&a->maxx, c.maxx);
    atomicMin(&a->miny, c.miny);
    atomicMax(&a->maxy, c.maxy);
}

// grid: (ceil(h*ww/256), n).  Per-segment contributions are first combined per label in a small LDS hash table
// (a block covers ~8 rows, so it sees a handful of labels), then each occupied slot is flushed with one set of
// global atomics.
#define ST_SLOTS 64
struct st_table {
    u32 label[ST_SLOTS];
    u32 area[ST_SLOTS];
    int minx[ST_SLOTS], maxx[ST_SLOTS], miny[ST_SLOTS], maxy[ST_SLOTS];
    u64 sx[ST_SLOTS], sy[ST_SLOTS];
};
__device__ __forceinline__ void ccl_stats_body(const u64* __restrict__ bits, const ccl_geom& G, const u32* __restrict__ parent,
                                               const u32* __restrict__ flags, const u32* __restrict__ prefix,
                                               u32* __restrict__ seglabel, u32* __restrict__ wordlabel,
                                               ccl_acc* __restrict__ acc, int max_labels, int vbx, int frame)
{
    __shared__ st_table T;
    const int idx = vbx * 256 + threadIdx.x;
    const bool live = idx < G.h * G.ww;
    const int f = frame;
    const u64 w = live ? bits[(size_t)f * G.h * G.ww + idx] : 0ull;
    const bool any_fg = __syncthreads_or(w != 0ull);   // block-uniform
    ccl_acc* a = acc + (size_t)f * max_labels;
    if (any_fg) {
        if (threadIdx.x < ST_SLOTS) {
            const int i = threadIdx.x;
            T.label[i] = 0; T.area[i] = 0; T.sx[i] = 0; T.sy[i] = 0;
            T.minx[i] = INT_MAX; T.miny[i] = INT_MAX; T.maxx[i] = INT_MIN; T.maxy[i] = INT_MIN;
        }
        __syncthreads();
        // label of a segment + its contribution; the first segment of every word goes through a wave-level shortcut: when all
        // the first segments of a wave carry the same label (the inside of a blob, a full mask) their records are combined with
        // shuffles and added once, instead of 64 lanes queueing on the same LDS slot
        const int y = idx / G.ww, j = idx - y * G.ww;
        const u32* p = parent + (size_t)f * G.nids;
        const u32* fl = flags + (size_t)f * G.nw32;
        const u32* pf = prefix + (size_t)f * G.nw32;
        u32* sl = seglabel + (size_t)f * G.nids;
        auto table_add = [&](u32 label, const contrib& c) {
            u32 slot = (label * 2654435761u) >> 26;   // 6 bits
            for (int probe = 0; probe < 8; probe++, slot = (slot + 1) & (ST_SLOTS - 1)) {
                const u32 cur = atomicCAS(&T.label[slot], 0u, label);
                if (cur == 0u || cur == label) {
                    atomicAdd(&T.area[slot], c.area);
                    atomicAdd((unsigned long long*)&T.sx[slot], (unsigned long long)c.sx);
                    atomicAdd((unsigned long long*)&T.sy[slot], (unsigned long long)c.sy);
                    atomicMin(&T.minx[slot], c.minx);
                    atomicMax(&T.maxx[slot], c.maxx);
                    atomicMin(&T.miny[slot], c.miny);
                    atomicMax(&T.maxy[slot], c.maxy);
                    return;
                }
            }
            acc_commit(a + label, c);   // crowded block (noise): straight to global memory
        };
        const bool multi = nstarts(w) > 1u;   // the label-write kernel reads seglabel only for words holding several segments
        auto lookup = [&](int s) -> u32 {     // label of the segment starting at bit s: four dependent, uncoalesced reads
            const u32 id = seg_id(G, y, 64 * j + s);
            u32 r = id;
            for (u32 q = p[r]; q != r; q = p[r]) r = q;   // read-only walk: strip root, then across strips
            const u32 label = pf[r >> 5] + (u32)__popc(fl[r >> 5] & ((1u << (r & 31)) - 1u)) + 1u;
            if (multi) sl[id] = label;
            return label;
        };
        auto record = [&](int s, int e, contrib& c) {
            const u32 len = (u32)(e - s + 1);
            const int xs = 64 * j + s, xe = 64 * j + e;
            c.area = len; c.sx = (u64)len * (u64)(xs + xe) / 2ull; c.sy = (u64)len * (u64)y;
            c.minx = xs; c.maxx = xe; c.miny = c.maxy = y;
        };
        u64 rem = w;
        contrib c0;
        contrib_zero(c0);
        u32 lab0 = 0;
        {
            // A first segment that continues the only segment of the word to its left (same row, same wave) has that segment's
            // label: only the first word of such a chain looks its label up, the others take it through a wave scan.  Inside
            // blobs that removes most of the uncoalesced reads this kernel waits for.
            const int lane = threadIdx.x & 63;
            const u64 wprev = __shfl_up(w, 1);
            bool take = (w & 1ull) && lane > 0 && j > 0 && (wprev >> 63) && nstarts(wprev) == 1u;
            int s0 = 0, e0 = 0;
            u32 lab = 0;
            if (w) {
                s0 = __ffsll((long long)rem) - 1;
                e0 = run_end(rem, s0);
                rem &= ~bit_range(s0, e0);
                if (!take) lab = lookup(s0);
            }
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const u32 pv = __shfl_up(lab, d);
                const int pt = __shfl_up((int)take, d);
                if (lane >= d && take) { lab = pv; take = pt != 0; }
            }
            if (w) {
                if (multi) sl[seg_id(G, y, 64 * j + s0)] = lab;
                wordlabel[(size_t)f * G.h * G.ww + idx] = lab;
                if (lab < (u32)max_labels) { lab0 = lab; record(s0, e0, c0); }
            }
        }
        const unsigned long long act = __ballot(lab0 != 0u);
        if (act) {
            const int lead = __ffsll((long long)act) - 1;
            const u32 ref = __shfl(lab0, lead);
            if (__popcll(act) >= 8 && __all(lab0 == 0u || lab0 == ref)) {
                wave_combine(c0);
                if ((int)(threadIdx.x & 63) == lead) table_add(ref, c0);
            } else if (lab0) {
                table_add(lab0, c0);
            }
        }
        while (rem) {
            const int s = __ffsll((long long)rem) - 1;
            const int e = run_end(rem, s);
            rem &= ~bit_range(s, e);
            contrib c;
            const u32 label = lookup(s);
            if (label < (u32)max_labels) { record(s, e, c); table_add(label, c); }
        }
        __syncthreads();
        if (threadIdx.x < ST_SLOTS && T.label[threadIdx.x]) {
            const int i = threadIdx.x;
            contrib c;
            c.area = T.area[i]; c.sx = T.sx[i]; c.sy = T.sy[i]; c.minx = T.minx[i]; c.maxx = T.maxx[i]; c.miny = T.miny[i]; c.maxy = T.maxy[i];
            acc_commit(a + T.label[i], c);
        }
    }
}
__global__ __launch_bounds__(256) void k_ccl_stats(const u64* __restrict__ bits, ccl_geom G, const u32* __restrict__ parent,
                                                   const u32* __restrict__ flags, const u32* __restrict__ prefix,
                                                   u32* __restrict__ seglabel, u32* __restrict__ wordlabel,
                                                   ccl_acc* __restrict__ acc, int max_labels, const u32* __restrict__ only)
{
    if (only && !only[blockIdx.y]) return;
    ccl_stats_body(bits, G, parent, flags, prefix, seglabel, wordlabel, acc, max_labels, (int)blockIdx.x, (int)blockIdx.y);
}

// grid: (ceil(max_labels/256), n); nl: the frame's label count
__device__ __forceinline__ void ccl_final_body(const ccl_acc* __restrict__ acc, const contrib* __restrict__ bgpart, int nl, int max_labels,
                                               int32_t* __restrict__ stats, double* __restrict__ cent, int vbx, int frame)
{
    const int l = vbx * 256 + threadIdx.x;
    if (l >= max_labels) return;
    const int f = frame;
    const size_t o = (size_t)f * max_labels + l;
    if (l < nl) {
        ccl_acc a = acc[o];
        if (l == 0) {   // background: merge the per-slice records
            contrib c;
            contrib_zero(c);
            for (int k = 0; k < BG_PARTS; k++) contrib_merge(c, bgpart[(size_t)f * BG_PARTS + k]);
            a.area = c.area; a.minx = c.minx; a.maxx = c.maxx; a.miny = c.miny; a.maxy = c.maxy; a.sx = c.sx; a.sy = c.sy;
        }
        if (stats) {
            int32_t* s = stats + o * 5;
            s[0] = a.minx;
            s[1] = a.miny;
            s[2] = (int32_t)((u32)a.maxx - (u32)a.minx + 1u);
            s[3] = (int32_t)((u32)a.maxy - (u32)a.miny + 1u);
            s[4] = (int32_t)a.area;
        }
        if (cent) {
            const double area = (double)a.area;
            cent[o * 2] = (double)a.sx / area;
            cent[o * 2 + 1] = (double)a.sy / area;
        }
    } else {
        if (stats) { int32_t* s = stats + o * 5; s[0] = s[1] = s[2] = s[3] = s[4] = 0; }
        if (cent) { cent[o * 2] = 0.0; cent[o * 2 + 1] = 0.0; }
    }
}
__global__ __launch_bounds__(256) void k_ccl_final(const ccl_acc* __restrict__ acc, const contrib* __restrict__ bgpart,
                                                   const int32_t* __restrict__ nlabels, int max_labels, int32_t* __restrict__ stats,
                                                   double* __restrict__ cent, const u32* __restrict__ only)
{
    if (only && !only[blockIdx.y]) return;
    ccl_final_body(acc, bgpart, nlabels[blockIdx.y], max_labels, stats, cent, (int)blockIdx.x, (int)blockIdx.y);
}

// ---- label image -------------------------------------------------------------------------------------------
// One lane = 4 px = one 16-B store.  A block streams WR_ROWS consecutive rows; a thread owns WR_K groups and runs
// in phases — all bit-word + word-label loads, then the stores — so that no load waits behind a store (vmcnt
// counts stores too on CDNA4).  A word with a single segment (the common case inside blobs) takes its label from
// the dense wordlabel array; only words holding several segments go to the sparse seglabel array.
// launch bound 8 waves per SIMD: the compiler otherwise takes 74 VGPRs (6 waves); at 62 VGPRs and full occupancy the kernel streams at
// 5.8 instead of 5.2 TB/s (188 instead of 208 us per 128 frames)
#define WR_K 8
// rows [row0, row0 + nrows) of the batch's (n * h) rows
__device__ __forceinline__ void ccl_write_body(const u64* __restrict__ bits, const ccl_geom& G, const u32* __restrict__ seglabel,
                                               const u32* __restrict__ wordlabel, int32_t* __restrict__ labels, u32 row0, u32 nrows,
                                               u32 gpr, u32 gpr_magic)
{
    const u32 ngroups = nrows * gpr;
    const bool vec = (G.w & 3) == 0 && ((((uintptr_t)labels) & 15) == 0);
    const u64* brow0 = bits + (size_t)row0 * G.ww;
    const u32* wrow0 = wordlabel + (size_t)row0 * G.ww;
    int32_t* lrow0 = labels + (size_t)row0 * G.w;
    const u32 f0 = row0 / (u32)G.h;
    const u32 y0 = row0 - f0 * (u32)G.h;
    for (u32 qb = 0; qb < ngroups; qb += 256 * WR_K) {
        u64 w[WR_K];
        u32 wl[WR_K], rl[WR_K], g[WR_K];
        bool live[WR_K];
#pragma unroll
        for (int k = 0; k < WR_K; k++) {
            const u32 q = qb + (u32)k * 256 + threadIdx.x;
            live[k] = q < ngroups;
            const u32 qq = live[k] ? q : 0;
            rl[k] = gpr == 1 ? qq : __umulhi(qq, gpr_magic);   // qq / gpr (exact for qq < 2^16 * gpr)
            g[k] = qq - rl[k] * gpr;
            const u32 wi = rl[k] * (u32)G.ww + (g[k] >> 4);
            w[k] = brow0[wi];
            wl[k] = wrow0[wi];
        }
        u32 la[WR_K], lb[WR_K], m1[WR_K], m2[WR_K];
        bool sparse = false;
#pragma unroll
        for (int k = 0; k < WR_K; k++) {
            const u32 nib = (u32)(w[k] >> ((g[k] * 4) & 63)) & 0xfu;
            m1[k] = nib;
            m2[k] = 0;
            la[k] = wl[k];
            lb[k] = 0;
            sparse |= nib && (nstarts(w[k]) > 1);
        }
        if (__any(sparse)) {   // wave-uniform, rare: some word here holds more than one segment
#pragma unroll
            for (int k = 0; k < WR_K; k++) {
                const u32 nib = m1[k];
                if (!nib || nstarts(w[k]) <= 1) continue;
                const int x0 = (int)g[k] * 4, sub = x0 & 63, j = x0 >> 6;
                u32 y = y0 + rl[k], f = f0;
                while (y >= (u32)G.h) { y -= (u32)G.h; f++; }
                const u32* sl = seglabel + (size_t)f * G.nids;
                // first run of the nibble, and what is left after it (at most one more run)
                const int tz = __ffs((int)nib) - 1;
                const u32 t = nib >> tz;
                const int runlen = __ffs((int)~t) - 1;
                m1[k] = ((1u << runlen) - 1u) << tz;
                m2[k] = nib & ~m1[k];
                la[k] = sl[seg_id(G, (int)y, 64 * j + run_start(w[k], sub + tz))];
                if (m2[k]) lb[k] = sl[seg_id(G, (int)y, 64 * j + sub + (__ffs((int)m2[k]) - 1))];
            }
        }
#pragma unroll
        for (int k = 0; k < WR_K; k++) {
            if (!live[k]) continue;
            const int x0 = (int)g[k] * 4;
            int vv[4];
#pragma unroll
            for (int b = 0; b < 4; b++) vv[b] = ((m1[k] >> b) & 1u) ? (int)la[k] : (((m2[k] >> b) & 1u) ? (int)lb[k] : 0);
            int32_t* d = lrow0 + (size_t)rl[k] * G.w + x0;
            if (vec && x0 + 4 <= G.w) {
                vp_store16(d, (u32)vv[0], (u32)vv[1], (u32)vv[2], (u32)vv[3]);
            } else {
                for (int b = 0; b < 4; b++)
                    if (x0 + b < G.w) d[b] = vv[b];
            }
        }
    }
}
__global__ __launch_bounds__(256, 8) void k_ccl_write(const u64* __restrict__ bits, ccl_geom G, const u32* __restrict__ seglabel,
                                                   const u32* __restrict__ wordlabel, int32_t* __restrict__ labels, u32 total_rows,
                                                   u32 gpr, u32 gpr_magic)
{
    const u32 row0 = blockIdx.x * WR_ROWS;
    ccl_write_body(bits, G, seglabel, wordlabel, labels, row0, min((u32)WR_ROWS, total_rows - row0), gpr, gpr_magic);
}

#ifdef VP_PROBE
static __device__ int vp_dbg_bits;   // the VP_DBG switches of this unit's kernels
static int g_dbg_bits_host;          // what vp_debug_set last set
#endif
#include "vp_ccl3.inl"
#include "vp_ccl2.inl"

// what the environment tunes of the plan and the grids (vp_ccl_plan.h), read on first use
static const ccl_tuning& ccl_env_tuning()
{
    static const ccl_tuning T = ccl_tuning_from_env();
    return T;
}

// union-find phase only: parent[] (every segment points at a smaller id of its component, roots at themselves)
// and the exact root bitmap in flags[]; `only` (nullable): per-frame switch, frames whose entry is 0 are left alone
// zero_too (nullable): a bitmap laid out like `flags` that the caller wants cleared (the strip kernel clears its slice of the root
// bitmap anyway; the contour code's "reaches the frame" bitmap rides along instead of costing a memset launch)
static int ccl_roots(vp_ctx* ctx, const u64* d_bits, const ccl_geom& G, int n, u32* parent, u32* flags, const u32* only = nullptr,
                     u32* zero_too = nullptr)
{
    const int h = G.h;
    const dim3 wgrid((unsigned)((h * G.ww + 255) / 256), (unsigned)n);
    hipStream_t s = ctx->stream;
    const int strips = (h + G.rows - 1) / G.rows;
    size_t cap;
    const size_t lds_local = ccl_local_lds(G, cap, ccl_env_tuning());
    if (lds_local <= 64 * 1024) {
        ctx->ccl.launches += strips > 1 ? 2 : 1;
        { vp_prof_scope ps(ctx, VPK_CCL_LOCAL); hipLaunchKernelGGL(k_ccl_local, dim3((unsigned)((size_t)n * strips)), dim3(256), lds_local, s, d_bits, G, parent, flags, strips, (int)cap, only, zero_too); }
        if (strips > 1) { vp_prof_scope ps(ctx, VPK_CCL_BOUNDARY); hipLaunchKernelGGL(k_ccl_boundary, dim3((unsigned)(strips - 1), (unsigned)n), dim3(64), 0, s, d_bits, G, parent, flags, only); }
    } else {
        if (zero_too) { vp_prof_scope ps(ctx, VPK_MEMSET); VP_HIP(ctx, hipMemsetAsync(zero_too, 0, (size_t)G.nw32 * 4 * n, s)); }
        { vp_prof_scope ps(ctx, VPK_MEMSET); VP_HIP(ctx, hipMemsetAsync(flags, 0, (size_t)G.nw32 * 4 * n, s)); }
        ctx->ccl.launches += 2;
        { vp_prof_scope ps(ctx, VPK_CCL_BOUNDARY); hipLaunchKernelGGL(k_ccl_init, wgrid, dim3(256), 0, s, d_bits, G, parent, flags); }
        { vp_prof_scope ps(ctx, VPK_CCL_LOCAL); hipLaunchKernelGGL(k_ccl_link, wgrid, dim3(256), 0, s, d_bits, G, parent, flags); }
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

// the one-level kernels after the union-find: ranks, per-label statistics, stats rows; on ctx->stream
static int ccl_one_level_tail(vp_ctx* ctx, const u64* d_bits, const ccl_geom& G, int n, const vp_ccl_ws& ws, int32_t* d_stats,
                              double* d_centroids, int max_labels, int32_t* d_nlabels, const u32* only)
{
    const dim3 wgrid((unsigned)((G.h * G.ww + 255) / 256), (unsigned)n);
    hipStream_t s = ctx->stream;
    ctx->ccl.launches += (d_stats || d_centroids) ? 3 : 2;
    { vp_prof_scope ps(ctx, VPK_CCL_RANK); hipLaunchKernelGGL(k_ccl_rank, dim3(RK_PARTS + BG_PARTS, (unsigned)n), dim3(256), 0, s, G, ws.flags, ws.prefix, d_nlabels, (ccl_acc*)ws.acc, max_labels, d_bits, (contrib*)ws.bgpart, only); }
    { vp_prof_scope ps(ctx, VPK_CCL_STATS); hipLaunchKernelGGL(k_ccl_stats, wgrid, dim3(256), 0, s, d_bits, G, ws.parent, ws.flags, ws.prefix, ws.seglabel, ws.wordlabel, (ccl_acc*)ws.acc, max_labels, only); }
    if (d_stats || d_centroids) {
        vp_prof_scope ps(ctx, VPK_CCL_FINAL);
        hipLaunchKernelGGL(k_ccl_final, dim3((unsigned)((max_labels + 255) / 256), (unsigned)n), dim3(256), 0, s, (const ccl_acc*)ws.acc,
                           (const contrib*)ws.bgpart, d_nlabels, max_labels, d_stats, d_centroids, only);
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

// ---- dispatch --------------------------------------------------------------------------------------------------------------
// vpk_ccl makes the plan (ccl_make_plan, vp_ccl_plan.h) and hands it to one launcher per path: ccl_two_level, which finishes the
// frames its merge hands over with ccl_crowded (or, while none is expected, with the one launch of k_ccl2_finish: vp_ccl_hint.h) or,
// where the geometry does not suit those kernels, with the one-level kernels (ccl_roots + ccl_one_level_tail); and the one-level
// path itself.

struct ccl_call {            // the arguments of vpk_ccl that the launchers pass on
    const u64* bits; int n; const vp_ccl_ws& ws; int32_t* labels; int32_t* stats; double* cent; int max_labels; int32_t* nlabels;
};

// Accumulators of the components that span strips, indexed by label: a set of the context's own that is all "empty" between calls -
// k_ccl3_rows resets exactly the entries it reads - so that no launch writes max_labels entries per frame (268 MB per 128 frames
// with 65,536 labels allowed: a quarter of what k_ccl3_link stored).  The set is clean only in the order of one stream and only once
// every launch of a call has been accepted: c3_acc_acquire marks it dirty, c3_acc_commit - after the call's last launch was taken -
// clean, and a dirty set is reinitialised before its next use.  *acc is left alone when the context has no set of `need` bytes
// (no memory): the caller then keeps the workspace's set and its clearing per call.
static int c3_acc_acquire(vp_ctx* ctx, size_t need, hipStream_t s, ccl_acc** acc)
{
    if (need > ctx->ccl.c3_acc_bytes) {
        VP_HIP(ctx, hipStreamSynchronize(s));
        if (ctx->ccl.c3_acc) { (void)hipFree(ctx->ccl.c3_acc); ctx->ccl.c3_acc = nullptr; ctx->ccl.c3_acc_bytes = 0; }
        if (hipMalloc(&ctx->ccl.c3_acc, need) == hipSuccess) { ctx->ccl.c3_acc_bytes = need; ctx->ccl.c3_acc_dirty = 1; }
        else (void)hipGetLastError();
    }
    if (!ctx->ccl.c3_acc || need > ctx->ccl.c3_acc_bytes) return VP_OK;
    if (ctx->ccl.c3_acc_dirty) {
        const size_t entries = ctx->ccl.c3_acc_bytes / sizeof(ccl_acc);
        hipLaunchKernelGGL(k_ccl3_acc_init, dim3((unsigned)std::min<size_t>((entries + 255) / 256, 65535)), dim3(256), 0, s, (ccl_acc*)ctx->ccl.c3_acc, entries);
    }
    ctx->ccl.c3_acc_dirty = 1;
    *acc = (ccl_acc*)ctx->ccl.c3_acc;
    return VP_OK;
}

// (LEAN mode, ccl_two_level, commits straight after acquiring: it launches nothing that touches the set, so the set is as clean as
// c3_acc_acquire left it - initialised in stream order - and there is no launch of its own to wait for.)
static void c3_acc_commit(vp_ctx* ctx)
{
#ifdef VP_PROBE
    if (g_dbg_bits_host) return;   // kernels that skip work do not hand every entry back clean
#endif
    ctx->ccl.c3_acc_dirty = 0;
}

// Kernels accept more dynamic LDS than the 64 KB default once told so - per device, hence remembered in the context (grow-only).
static bool c3_allow_lds(const void* kernel, size_t lds, size_t& allowed)
{
    if (lds <= allowed) return true;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) { (void)hipGetLastError(); return false; }
    allowed = lds;
    return true;
}

// K = 1: strips of up to 8192 ids; K = 2: taller strips, twice the threads per block.  The light labelling instantiation always has
// 512 threads: at ~120 registers a CU holds 16 waves, i.e. two blocks of eight.
template <int K>
static bool c3_allow_plan_lds(vp_ctx* ctx, const ccl_plan& P)
{
    size_t* set = ctx->ccl.c3_lds_set;
    return c3_allow_lds((const void*)k_ccl3_link<K * C3_LINK_THREADS>, P.lds3a, set[2 * (K - 1)]) &&
           c3_allow_lds((const void*)k_ccl3_label<K * C3_LABEL_THREADS, 0, C3_ACC>, P.lds3b, set[2 * (K - 1) + 1]) &&
           c3_allow_lds((const void*)k_ccl3_label<C3_LABEL_THREADS, C3_LIGHT_ROOTS, C3_LIGHT_ACC>, P.lds3c, set[4]);
}

// The crowded-frame kernels (vp_ccl3.inl): launches that read the list of handed-over frames and leave at once when it is empty (the
// usual case).
template <int K>
// prepare: the one run on an empty list that ccl_prepare_crowded queues (ncrowded then points at a zero word): nothing is acquired,
// counted or written.
static int ccl_crowded(vp_ctx* ctx, const ccl_plan& P, const ccl_call& c, u32* hint, const u32* ncrowded, bool prepare = false)
{
    const ccl_tuning& T = ccl_env_tuning();
    const ccl_geom& G = P.G;
    const c3_plan& P3 = P.P3;
    const vp_ccl_ws& ws = c.ws;
    hipStream_t s = ctx->stream;
    const int scap = (int)c3_strips_cap(G.h);
    ccl_acc* acc3 = (ccl_acc*)ws.acc;
    if (ctx->opt.v[VP_OPT_CHAIN_STREAMS] == 1 && !prepare) {   // sub-batches on several streams would share the context's set: they keep the workspace's
        const int rc = c3_acc_acquire(ctx, sizeof(ccl_acc) * (size_t)c.max_labels * (size_t)c.n, s, &acc3);
        if (rc != VP_OK) return rc;
    }
    const bool acc3_own = acc3 != (ccl_acc*)ws.acc;
    { vp_prof_scope ps(ctx, VPK_CCL_LOCAL);
      hipLaunchKernelGGL(k_ccl3_link<K * C3_LINK_THREADS>, dim3((unsigned)(ctx->num_cu * T.lgrid)), dim3(K * C3_LINK_THREADS), P.lds3a, s, c.bits, G, P3, ncrowded,
                         ws.c3_clist, ws.parent, ws.flags, ws.c3_child, ws.c3_lroot, ws.seglabel, acc3, c.max_labels, acc3_own ? 0 : 1, hint); }
    { vp_prof_scope ps(ctx, VPK_CCL_BOUNDARY);
      const size_t span = (size_t)2 * G.wb + 4;     // u16 roots of the two rows (row pairs) that meet: span entries each
      hipLaunchKernelGGL(k_ccl3_bound, dim3((unsigned)(ctx->num_cu * T.bgrid)), dim3(256), span * 4 + 16, s, c.bits, G, P3, ncrowded, ws.c3_clist, ws.parent, ws.flags,
                         ws.c3_child, ws.seglabel); }
    { vp_prof_scope ps(ctx, VPK_CCL_RANK);
      hipLaunchKernelGGL(k_ccl3_rank, dim3((unsigned)(ctx->num_cu * 4)), dim3(256), 0, s, G, P3, ncrowded, ws.c3_clist, ws.flags, ws.prefix, ws.c3_barr, ws.c3_lroot, ws.parent,
                         ws.c3_items); }
    { vp_prof_scope ps(ctx, VPK_CCL_STATS);
      // two instantiations, each taking the strips k_ccl3_rank marked for it: LIGHT first - two blocks per CU - then HEAVY
      auto label = [&](auto kernel, int blocks_per_cu, int threads, size_t lds) {
          hipLaunchKernelGGL(kernel, dim3((unsigned)(ctx->num_cu * blocks_per_cu)), dim3(threads), lds, s, c.bits, G, P3, ncrowded, ws.c3_items, ws.c3_clist, ws.parent,
                             ws.flags, ws.c3_child, ws.prefix, ws.c3_lroot, ws.seglabel, ws.c3_barr, (c3_state*)ws.c3_state, (contrib*)ws.c3_tot, scap, c.nlabels, acc3,
                             c.max_labels, c.labels, c.stats, c.cent);
      };
      label(k_ccl3_label<C3_LABEL_THREADS, C3_LIGHT_ROOTS, C3_LIGHT_ACC>, T.agrid_light, C3_LABEL_THREADS, P.lds3c);
      label(k_ccl3_label<K * C3_LABEL_THREADS, 0, C3_ACC>, T.agrid, K * C3_LABEL_THREADS, P.lds3b); }
    if (!prepare) ctx->ccl.launches += 5;
    if (c.stats || c.cent || acc3_own) {
        if (!prepare) ctx->ccl.launches++;
        vp_prof_scope ps(ctx, VPK_CCL_FINAL);
        hipLaunchKernelGGL(k_ccl3_rows, dim3((unsigned)(ctx->num_cu * 4)), dim3(256), 0, s, G, P3, ncrowded, ws.c3_clist, ws.flags, ws.c3_child, ws.prefix,
                           ws.c3_barr, (const c3_state*)ws.c3_state, (const contrib*)ws.c3_tot, scap, acc3, c.max_labels, c.stats, c.cent, acc3_own ? 1 : 0);
    }
    VP_HIP(ctx, hipGetLastError());
    if (acc3_own) c3_acc_commit(ctx);   // every launch was taken: k_ccl3_rows hands back clean every entry the labelling launches touch
    return VP_OK;
}

// The context's hint word (vp_ccl_hint.h): pinned host memory the device writes and the host reads without synchronising, made on the
// first two-level call.  Null when it could not be made: the labelling then always queues the crowded-frame kernels.
static u32* ccl_hint_word(vp_ctx* ctx)
{
    if (!ctx->ccl.hint_host && !ctx->ccl.hint_failed) {
        void* p = nullptr;
        if (hipHostMalloc(&p, sizeof(u32), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); ctx->ccl.hint_failed = 1; return nullptr; }
        *(volatile u32*)p = 0u;
        ctx->ccl.hint_host = (uint32_t*)p;
    }
    return ctx->ccl.hint_host;
}

// A process that has only run LEAN has never dispatched the crowded-frame kernels, and the call that switches to FULL - in the middle of
// a crowded run - paid for their first dispatch: ~0.2 ms once per process on top of that call (EXPERIMENTS.md).  The first LEAN call of a
// context for either strip height therefore queues them once on an empty list (a zero word of the context's in place of the merge's
// count; six launches that leave at once, ~17 us, never again).  Not part of the labelling sequence vp_ccl_last_launches counts.
static int ccl_prepare_crowded(vp_ctx* ctx, const ccl_plan& P, const ccl_call& c)
{
    int& d = ctx->ccl.prepared[P.c3_tall ? 1 : 0];   // per context: a superset of per process and per device, and free of races
    if (d) return VP_OK;
    if (!ctx->ccl.zero_dev) {
        void* p = nullptr;
        if (hipMalloc(&p, 256) != hipSuccess) { (void)hipGetLastError(); return VP_OK; }
        if (hipMemsetAsync(p, 0, 256, ctx->stream) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(p); return VP_OK; }
        ctx->ccl.zero_dev = (u32*)p;
    }
    d = 1;
    return P.c3_tall ? ccl_crowded<2>(ctx, P, c, nullptr, ctx->ccl.zero_dev, true) : ccl_crowded<1>(ctx, P, c, nullptr, ctx->ccl.zero_dev, true);
}

// what c3_acc_acquire, ccl_hint_word and ccl_prepare_crowded made (vp_destroy; the context's stream is idle)
void vp_ccl_teardown(vp_ctx* ctx)
{
    if (ctx->ccl.c3_acc) (void)hipFree(ctx->ccl.c3_acc);
    if (ctx->ccl.hint_host) (void)hipHostFree(ctx->ccl.hint_host);
    if (ctx->ccl.zero_dev) (void)hipFree(ctx->ccl.zero_dev);
    ctx->ccl = vp_ccl_state{};
}

// The two-level path (vp_ccl2.inl): strips resolved in LDS, one merge block per frame; frames the merge hands over go to the
// crowded-frame kernels when the geometry suits them (it does for every frame up to 8192 px wide) and the device allows their LDS,
// otherwise to the one-level kernels.  Where the crowded-frame kernels serve, the hint of an earlier call decides whether they are
// queued at all (FULL) or one launch of k_ccl2_finish stands behind the merge in their place (LEAN): the results are the same.
static int ccl_two_level(vp_ctx* ctx, const ccl_plan& P, const ccl_call& c)
{
    const ccl_geom& G = P.G;
    const vp_ccl_ws& ws = c.ws;
    hipStream_t s = ctx->stream;
    const int n = c.n;
    const bool c3_ok = P.P3.ok && (P.c3_tall ? c3_allow_plan_lds<2>(ctx, P) : c3_allow_plan_lds<1>(ctx, P));
    const int c3_strips = c3_ok ? P.P3.strips : 0;
    int mode = CCL_MODE_FULL;
    u32* hint = nullptr;
    if (c3_ok && (hint = ccl_hint_word(ctx)) != nullptr) {
        ccl_hint_state st = {ctx->ccl.hint_mode, ctx->ccl.hint_quiet};
        mode = ccl_hint_decide(st, *(volatile u32*)hint, ctx->opt.v[VP_OPT_CCL_CROWDED], ctx->opt.v[VP_OPT_CHAIN_STREAMS] + (ctx->ccl.beside ? 1 : 0));
        ctx->ccl.hint_mode = st.mode; ctx->ccl.hint_quiet = st.quiet;
    }
    ctx->ccl.launches += 2;
    { vp_prof_scope ps(ctx, VPK_CCL2_LOCAL);
      hipLaunchKernelGGL(k_ccl2_local, dim3((unsigned)((size_t)n * P.strips)), dim3(256), P.lds2, s, c.bits, G, P.strips, (int)P.cap2, (int)P.rc, (int)P.tail_words, ws.c2_ncomp,
                         (contrib*)ws.c2_recs, (c2_box*)ws.c2_bgbox, ws.wordlabel, ws.seglabel, ws.c3_ncrowded); }
    { vp_prof_scope ps(ctx, VPK_CCL2_MERGE);
      hipLaunchKernelGGL(k_ccl2_merge, dim3((unsigned)n), dim3(C2_THREADS), 0, s, c.bits, G, P.strips, P.mcap, ws.c2_ncomp, (const contrib*)ws.c2_recs,
                         (const c2_box*)ws.c2_bgbox, ws.wordlabel, ws.seglabel, ws.c2_label, ws.c2_crowded, c.nlabels, c.stats, c.cent, c.max_labels,
                         ws.c3_ncrowded, ws.c3_clist, (c3_state*)ws.c3_state, ws.c3_barr, c3_strips); }
    VP_HIP(ctx, hipGetLastError());
    int rc = VP_OK;
    if (c3_ok && mode == CCL_MODE_LEAN) {
        // The crowded-frame kernels' accumulator set is made and initialised here as well, though k_ccl2_finish works on the workspace's
        // accumulators and leaves the set alone (hence the commit at once: it is as clean as it was): the call that switches to FULL then
        // finds it ready instead of paying a synchronisation, hipMalloc and the set's initialisation (200 MB for 32 frames of 131,072
        // labels: 0.64 ms, measured as the first timed step of bench.py's s3_noise_labelling).
        rc = ccl_prepare_crowded(ctx, P, c);
        if (rc != VP_OK) return rc;
        ccl_acc* set = nullptr;
        rc = c3_acc_acquire(ctx, sizeof(ccl_acc) * (size_t)c.max_labels * (size_t)n, s, &set);
        if (rc != VP_OK) return rc;
        if (set) c3_acc_commit(ctx);
        ctx->ccl.launches++;
        vp_prof_scope ps(ctx, VPK_CCL_STATS);
        hipLaunchKernelGGL(k_ccl2_finish, dim3((unsigned)n), dim3(256), 0, s, c.bits, G, ws.c2_crowded, ws.c3_ncrowded, hint, ws.parent, ws.flags, ws.prefix,
                           (ccl_acc*)ws.acc, (contrib*)ws.bgpart, ws.seglabel, ws.wordlabel, c.nlabels, c.max_labels, c.labels, c.stats, c.cent, P.gpr, P.magic);
    } else if (c3_ok) {
        rc = P.c3_tall ? ccl_crowded<2>(ctx, P, c, hint, ws.c3_ncrowded) : ccl_crowded<1>(ctx, P, c, hint, ws.c3_ncrowded);
    } else {
        // the one-level kernels, launched whatever the frames hold (the flags live on the device); they leave at once for frames the merge resolved
        rc = ccl_roots(ctx, c.bits, G, n, ws.parent, ws.flags, ws.c2_crowded);
        if (rc == VP_OK) rc = ccl_one_level_tail(ctx, c.bits, G, n, ws, c.stats, c.cent, c.max_labels, c.nlabels, ws.c2_crowded);
    }
    if (rc != VP_OK) return rc;
    if (c.labels) {
        ctx->ccl.launches++;
        vp_prof_scope ps(ctx, VPK_CCL2_WRITE);
        const dim3 wr_grid((unsigned)((G.h + WR_ROWS - 1) / WR_ROWS), (unsigned)n);
        hipLaunchKernelGGL(k_ccl2_write<0>, wr_grid, dim3(256), 0, s, c.bits, G, P.strips, (int)P.rc, ws.seglabel, ws.wordlabel, ws.c2_label, ws.c2_crowded, c.labels, P.gpr, P.magic,
                           c3_ok ? 1 : 0);
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

int vpk_ccl(vp_ctx* ctx, const u64* d_bits, int w, int h, int n, int numbering, const vp_ccl_ws& ws, int32_t* d_labels,
            int32_t* d_stats, double* d_centroids, int max_labels, int32_t* d_nlabels)
{
    if (numbering != VP_CCL_BLOCK2X2 && numbering != VP_CCL_PIXEL) return vp_fail(ctx, VP_ERR_INVALID, "numbering");
    if (max_labels < 1) return vp_fail(ctx, VP_ERR_INVALID, "max_labels");
    const ccl_plan P = ccl_make_plan(w, h, numbering, ctx->opt.v[VP_OPT_CCL_LEVELS], ctx->opt.v[VP_OPT_CCL_MERGE_CAP], ccl_env_tuning());
    const ccl_call c = {d_bits, n, ws, d_labels, d_stats, d_centroids, max_labels, d_nlabels};
    ctx->ccl.launches = 0;   // kernels of the labelling sequence this call queues (vp_ccl_last_launches)
    if (P.two_level) return ccl_two_level(ctx, P, c);

    int rc = ccl_roots(ctx, d_bits, P.G, n, ws.parent, ws.flags);
    if (rc != VP_OK) return rc;
    rc = ccl_one_level_tail(ctx, d_bits, P.G, n, ws, d_stats, d_centroids, max_labels, d_nlabels, nullptr);
    if (rc != VP_OK) return rc;
    if (d_labels) {
        ctx->ccl.launches++;
        vp_prof_scope ps(ctx, VPK_CCL_WRITE);
        const u32 total_rows = (u32)((size_t)n * h);
        hipLaunchKernelGGL(k_ccl_write, dim3((total_rows + WR_ROWS - 1) / WR_ROWS), dim3(256), 0, ctx->stream, d_bits, P.G, ws.seglabel, ws.wordlabel, d_labels,
                           total_rows, P.gpr, P.magic);
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

#ifdef VP_PROBE
// measurement builds: the VP_DBG_* switches of vp_internal.h, for the kernels of this unit and of vp_morph.hip
extern "C" int vp_debug_set(int bits)
{
    g_dbg_bits_host = bits;
    if (hipMemcpyToSymbol(HIP_SYMBOL(vp_dbg_bits), &bits, sizeof bits) != hipSuccess) return -1;
    return vp_morph_debug_set(bits);
}

// per probe point, the ticks summed over the blocks that reached point 15 (ran to the end) in out[k*16 + i],
// their number in out[k*16 + 15]; slots are cleared afterwards
extern "C" int vp_debug_probe(double* out32)
{
    static std::vector<unsigned int> h((size_t)2 * C2_PROBE_BLOCKS * 16);
    if (hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(g_c2_probe), h.size() * 4) != hipSuccess) return -1;
    for (int i = 0; i < 32; i++) out32[i] = 0;
    for (int k = 0; k < 2; k++)
        for (int b = 0; b < C2_PROBE_BLOCKS; b++) {
            const unsigned int* r = &h[((size_t)k * C2_PROBE_BLOCKS + b) * 16];
            if (r[15] == 0xffffffffu || r[14] != 0x600dc0deu) continue;
            for (int i = 0; i < 14; i++) out32[k * 16 + i] += r[i];
            out32[k * 16 + 15] += 1;
        }
    std::fill(h.begin(), h.end(), 0u);
    return hipMemcpyToSymbol(HIP_SYMBOL(g_c2_probe), h.data(), h.size() * 4) == hipSuccess ? 0 : -1;
}

// crowded-frame kernels (link, bound, label): out[k * 16 + i] = ticks (10 ns) of phase i summed over blocks and items, out[k * 16 + 15] = blocks that ran
extern "C" int vp_debug_probe3(double* out32 /* 48 */)
{
    static std::vector<unsigned long long> h((size_t)3 * 2048 * 16);
    if (hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(g_c3_probe), h.size() * 8) != hipSuccess) return -1;
    for (int i = 0; i < 48; i++) out32[i] = 0;
    for (int k = 0; k < 3; k++)
        for (int b = 0; b < 2048; b++) {
            const unsigned long long* r = &h[((size_t)k * 2048 + b) * 16];
            unsigned long long t = 0;
            for (int i = 0; i < 15; i++) { out32[k * 16 + i] += (double)r[i]; t += r[i]; }
            if (t) out32[k * 16 + 15] += 1;
        }
    std::fill(h.begin(), h.end(), 0ull);
    return hipMemcpyToSymbol(HIP_SYMBOL(g_c3_probe), h.data(), h.size() * 8) == hipSuccess ? 0 : -1;
}
#endif

#include "vp_contours.inl"
