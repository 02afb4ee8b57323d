// Contour geometry: perimeter, convex hull, minimum-area rectangle and minimum enclosing circle of every
// contour of a point block in one launch.  One wave owns one contour, whatever its size: lanes stride its points, reductions are
// shuffles, the hull candidates live in the wave's LDS.  Every size and every shared formula comes from vp_geometry_plan.h; the rows
// that leave here are raw (integers and vertices), and one host function per descriptor finishes them (vp_api_geometry.hip).
#include "vp_internal.h"
#include "vp_geometry_plan.h"
#include <limits.h>

namespace {

struct geom_src {
    // flat form: contour r is counts[r] points from point first[r] of pts
    const int32_t* pts;
    const long long* first;
    const int32_t* counts;
    // batch form (info != nullptr): the buffers of vp_chain_run_contours; contour r of frame f
    const int32_t* info;
    const int32_t* offsets;
    int max_contours;
    long long max_points;
};

__device__ __forceinline__ u64 wave_min(u64 v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const u64 o = __shfl_xor(v, d); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ u64 wave_max(u64 v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const u64 o = __shfl_xor(v, d); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ long long wave_sum(long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__device__ __forceinline__ void zero_row(vp_geom_raw* o, uint32_t status)
{
    o->perim_units = 0; o->hull_area2 = 0; o->close_root = 0.f; o->hull_count = 0; o->status = status;
    for (int k = 0; k < 4; k++) o->edge[k] = 0;
    for (int k = 0; k < 8; k++) o->ext[k] = 0;
    for (int k = 0; k < 6; k++) o->sup[k] = 0;
}

// grid (contours, frames), GEOM_TB threads = one wave
__global__ __launch_bounds__(GEOM_TB) void k_geometry(geom_src S, vp_geom_raw* __restrict__ rows, int32_t* __restrict__ hull_out)
{
    __shared__ uint32_t s_key[GEOM_HULL_CAP + 8];   // candidates, sorted; then the hull (the chain's stack holds one entry more than the hull)
    __shared__ uint32_t s_uq[GEOM_HULL_CAP];        // the distinct candidates, in order
    __shared__ int s_h;
    const int lane = threadIdx.x;
    const size_t r = blockIdx.x, f = blockIdx.y;
    vp_geom_raw* o;
    const int32_t* p;
    int cnt;
    bool skipped = false;
    if (S.info) {
        o = rows + f * (size_t)S.max_contours + r;
        const int K = min(S.info[2 * f], S.max_contours);
        cnt = (long long)r < K ? S.counts[f * (size_t)S.max_contours + r] : -1;
        const long long off = (long long)r < K ? S.offsets[f * (size_t)S.max_contours + r] : 0;
        skipped = cnt <= 0 || off < 0 || off + cnt > S.max_points;
        p = S.pts + 2 * (f * (size_t)S.max_points + (size_t)(skipped ? 0 : off));
    } else {
        o = rows + r;
        cnt = S.counts[r];
        skipped = cnt < 0;
        p = S.pts + 2 * (size_t)(skipped ? 0 : S.first[r]);
    }
    if (skipped || cnt == 0) {
        if (lane == 0) zero_row(o, skipped ? GEOM_ST_SKIPPED : GEOM_ST_OK);
        return;
    }
    const int2* q = reinterpret_cast<const int2*>(p);

    // ---- pass 1: perimeter units and the eight extreme points -------------------------------------------------------------------
    long long units = 0;
    float close_root = 0.f;
    bool bad = false;
    u64 mnx = ~0ull, mny = ~0ull, mns = ~0ull, mnd = ~0ull, mxx = 0, mxy = 0, mxs = 0, mxd = 0;
    for (int i = lane; i < cnt; i += GEOM_TB) {
        const int2 a = q[i], b = q[i == 0 ? cnt - 1 : i - 1];
        if (a.x < GEOM_COORD_MIN || a.x > GEOM_COORD_MAX || a.y < GEOM_COORD_MIN || a.y > GEOM_COORD_MAX) { bad = true; continue; }
        if (b.x < GEOM_COORD_MIN || b.x > GEOM_COORD_MAX || b.y < GEOM_COORD_MIN || b.y > GEOM_COORD_MAX) { bad = true; continue; }
        const float root = vp_geom_seg_root(a.x - b.x, a.y - b.y);
        units += vp_geom_root_units(root);
        if (i == 0) close_root = root;
        const u64 pk = vp_geom_pack(a.x, a.y);
        const u64 kx = ((u64)(a.x + 32768) << 32) | pk, ky = ((u64)(a.y + 32768) << 32) | pk;
        const u64 ks = ((u64)(a.x + a.y + 65536) << 32) | pk, kd = ((u64)(a.x - a.y + 65536) << 32) | pk;
        mnx = kx < mnx ? kx : mnx; mxx = kx > mxx ? kx : mxx;
        mny = ky < mny ? ky : mny; mxy = ky > mxy ? ky : mxy;
        mns = ks < mns ? ks : mns; mxs = ks > mxs ? ks : mxs;
        mnd = kd < mnd ? kd : mnd; mxd = kd > mxd ? kd : mxd;
    }
    if (__any(bad)) {
        if (lane == 0) zero_row(o, GEOM_ST_COORD);
        return;
    }
    units = wave_sum(units);
    close_root = __shfl(close_root, 0);
    mnx = wave_min(mnx); mny = wave_min(mny); mns = wave_min(mns); mnd = wave_min(mnd);
    mxx = wave_max(mxx); mxy = wave_max(mxy); mxs = wave_max(mxs); mxd = wave_max(mxd);
    uint32_t status = units >= GEOM_PERIM_UNITS_MAX ? GEOM_ST_PERIMETER : GEOM_ST_OK;

    // the octagon, counter-clockwise by direction: +x, +x+y, +y, -x+y, -x, -x-y, -y, +x-y.  Support points of directions in angular
    // order come in boundary order, whichever of several tied points each reduction picked, so the polygon is (weakly) convex.
    const uint32_t oct[8] = {(uint32_t)mxx, (uint32_t)mxs, (uint32_t)mxy, (uint32_t)mnd, (uint32_t)mnx, (uint32_t)mns, (uint32_t)mny, (uint32_t)mxd};
    int ox[8], oy[8];
    bool any_edge = false;
#pragma unroll
    for (int k = 0; k < 8; k++) { ox[k] = vp_geom_px(oct[k]); oy[k] = vp_geom_py(oct[k]); }
#pragma unroll
    for (int k = 0; k < 8; k++) any_edge |= oct[k] != oct[(k + 1) & 7];

    // ---- pass 2: the points not strictly inside the octagon, compacted into LDS ----------------------------------------------------
    int m = 0;
    for (int base = 0; base < cnt; base += GEOM_TB) {
        const int i = base + lane;
        bool keep = false;
        uint32_t pk = 0;
        if (i < cnt) {
            const int2 a = q[i];
            pk = vp_geom_pack(a.x, a.y);
            bool inside = any_edge;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int k1 = (k + 1) & 7;
                if (oct[k] != oct[k1]) inside &= vp_geom_cross(ox[k], oy[k], ox[k1], oy[k1], a.x, a.y) > 0;
            }
            keep = !inside;
        }
        const u64 bal = __ballot(keep);
        const int slot = m + __popcll(bal & ((1ull << lane) - 1ull));
        if (keep && slot < GEOM_HULL_CAP) s_key[slot] = pk;
        m += __popcll(bal);
    }
    if (m > GEOM_HULL_CAP) {
        if (lane == 0) {
            zero_row(o, status | GEOM_ST_HULL_CAP);
            o->perim_units = units;
            o->close_root = close_root;
        }
        return;
    }
    __syncthreads();

    // ---- sort (bitonic network over the next power of two), drop duplicates ----------------------------------------------------------
    int n2 = 1;
    while (n2 < m) n2 <<= 1;
    for (int i = m + lane; i < n2; i += GEOM_TB) s_key[i] = 0xffffffffu;   // sorts behind every point (or equal to the largest one)
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (n2 >> 1); t += GEOM_TB) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const uint32_t a = s_key[i], b = s_key[l];
                const bool up = (i & k) == 0;
                if ((a > b) == up && a != b) { s_key[i] = b; s_key[l] = a; }
            }
            __syncthreads();
        }
    }
    int u = 0;
    for (int base = 0; base < m; base += GEOM_TB) {
        const int i = base + lane;
        bool uniq = false;
        uint32_t v = 0;
        if (i < m) { v = s_key[i]; uniq = i == 0 || s_key[i - 1] != v; }
        const u64 bal = __ballot(uniq);
        if (uniq) s_uq[u + __popcll(bal & ((1ull << lane) - 1ull))] = v;
        u += __popcll(bal);
    }
    __syncthreads();

    // ---- monotone chain (vp_convex_hull_i32's: collinear points dropped, from the smallest point, lower chain first) -------------------
    if (u <= 2) {
        if (lane < u) s_key[lane] = s_uq[lane];
        if (lane == 0) s_h = u;
    } else if (lane == 0) {
        int k = 0;
        for (int i = 0; i < u; i++) {
            const uint32_t c = s_uq[i];
            while (k >= 2 && vp_geom_cross(vp_geom_px(s_key[k - 2]), vp_geom_py(s_key[k - 2]), vp_geom_px(s_key[k - 1]), vp_geom_py(s_key[k - 1]),
                                           vp_geom_px(c), vp_geom_py(c)) <= 0) k--;
            s_key[k++] = c;
        }
        const int t = k + 1;
        for (int i = u - 2; i >= 0; i--) {
            const uint32_t c = s_uq[i];
            while (k >= t && vp_geom_cross(vp_geom_px(s_key[k - 2]), vp_geom_py(s_key[k - 2]), vp_geom_px(s_key[k - 1]), vp_geom_py(s_key[k - 1]),
                                           vp_geom_px(c), vp_geom_py(c)) <= 0) k--;
            s_key[k++] = c;
        }
        s_h = k - 1;    // the last entry is the first point again
    }
    __syncthreads();
    const int h = s_h;

    // ---- hull area and vertices -------------------------------------------------------------------------------------------------------
    long long area2 = 0;
    for (int i = lane; i < h; i += GEOM_TB) {
        const uint32_t a = s_key[i], b = s_key[i + 1 == h ? 0 : i + 1];
        area2 += (long long)vp_geom_px(a) * vp_geom_py(b) - (long long)vp_geom_px(b) * vp_geom_py(a);
        if (hull_out) {
            int32_t* ho = hull_out + (p - S.pts);
            ho[2 * i] = vp_geom_px(a);
            ho[2 * i + 1] = vp_geom_py(a);
        }
    }
    area2 = wave_sum(area2);
    if (area2 < 0) area2 = -area2;

    // ---- calipers: lanes over hull edges, each scanning the hull in vertex order; least area, then lowest edge ----------------------------
    double best_area = __builtin_huge_val();
    int best_edge = INT_MAX, b0 = 0, b1 = 0, b2 = 0, b3 = 0;
    if (h >= 2) {
        const vp_geom_hull_packed H = {s_key};
        const int edges = h > 2 ? h : 1;
        for (int e = lane; e < edges; e += GEOM_TB) {
            double ext[4];
            int arg[4];
            if (!vp_geom_edge_extents(H, h, e, ext, arg)) continue;
            const double wd = ext[0] - ext[1], ht = ext[2] - ext[3];
            const double area = wd * ht;
            if (best_edge == INT_MAX || area < best_area) { best_area = area; best_edge = e; b0 = arg[0]; b1 = arg[1]; b2 = arg[2]; b3 = arg[3]; }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const double oa = __shfl_xor(best_area, d);
            const int oe = __shfl_xor(best_edge, d), o0 = __shfl_xor(b0, d), o1 = __shfl_xor(b1, d), o2 = __shfl_xor(b2, d), o3 = __shfl_xor(b3, d);
            const bool take = oe != INT_MAX && (best_edge == INT_MAX || oa < best_area || (oa == best_area && oe < best_edge));
            if (take) { best_area = oa; best_edge = oe; b0 = o0; b1 = o1; b2 = o2; b3 = o3; }
        }
    }

    // ---- enclosing circle over the hull vertices: the incremental algorithm with exact predicates; "the first vertex outside the
    // current circle" is a ballot over the lanes, so the lowest index wins and the run is deterministic ------------------------------------
    vp_geom_support C;
    C.n = 0;
    for (int k = 0; k < 3; k++) C.x[k] = C.y[k] = 0;
    const int stride = vp_geom_stride(h);
    auto vx = [&](int t) { return s_key[(int)(((long long)t * stride) % h)]; };
    auto first_outside = [&](int lo, int hi) {
        for (int base = lo; base < hi; base += GEOM_TB) {
            const int t = base + lane;
            bool out = false;
            if (t < hi) { const uint32_t v = vx(t); out = vp_geom_outside(C, vp_geom_px(v), vp_geom_py(v)); }
            const u64 bal = __ballot(out);
            if (bal) return base + (int)__ffsll((long long)bal) - 1;
        }
        return hi;
    };
    if (h >= 1) {
        const uint32_t v0 = vx(0);
        C.n = 1; C.x[0] = vp_geom_px(v0); C.y[0] = vp_geom_py(v0);
        for (int i = first_outside(1, h); i < h; i = first_outside(i + 1, h)) {
            const uint32_t vi = vx(i);
            C.n = 1; C.x[0] = vp_geom_px(vi); C.y[0] = vp_geom_py(vi);
            for (int j = first_outside(0, i); j < i; j = first_outside(j + 1, i)) {
                const uint32_t vj = vx(j);
                C.n = 2; C.x[1] = vp_geom_px(vj); C.y[1] = vp_geom_py(vj);
                for (int k = first_outside(0, j); k < j; k = first_outside(k + 1, j)) {
                    const uint32_t vk = vx(k);
                    C.n = 3; C.x[2] = vp_geom_px(vk); C.y[2] = vp_geom_py(vk);
                }
            }
        }
    }

    if (lane == 0) {
        o->perim_units = units;
        o->hull_area2 = area2;
        o->close_root = close_root;
        o->hull_count = h;
        o->status = status | ((uint32_t)C.n << 8);
        if (h >= 2 && best_edge != INT_MAX) {     // (distinct vertices: every edge has a length, so some edge always wins)
            const uint32_t e0 = s_key[best_edge], e1 = s_key[(best_edge + 1) % h];
            o->edge[0] = (int16_t)vp_geom_px(e0); o->edge[1] = (int16_t)vp_geom_py(e0);
            o->edge[2] = (int16_t)vp_geom_px(e1); o->edge[3] = (int16_t)vp_geom_py(e1);
            const int bi[4] = {b0, b1, b2, b3};
            for (int k = 0; k < 4; k++) { const uint32_t v = s_key[bi[k]]; o->ext[2 * k] = (int16_t)vp_geom_px(v); o->ext[2 * k + 1] = (int16_t)vp_geom_py(v); }
        } else {
            const uint32_t e0 = s_key[0];
            o->edge[0] = o->edge[2] = (int16_t)vp_geom_px(e0); o->edge[1] = o->edge[3] = (int16_t)vp_geom_py(e0);
            for (int k = 0; k < 8; k++) o->ext[k] = 0;
        }
        for (int k = 0; k < 3; k++) { o->sup[2 * k] = (int16_t)C.x[k]; o->sup[2 * k + 1] = (int16_t)C.y[k]; }
    }
}

}  // namespace

int vpk_contour_geometry(vp_ctx* ctx, const int32_t* d_pts, const long long* d_first, const int32_t* d_counts, int n_contours, vp_geom_raw* d_rows,
                         int32_t* d_hull)
{
    if (n_contours <= 0) return VP_OK;
    vp_prof_scope ps(ctx, VPK_OTHER);
    geom_src S = {d_pts, d_first, d_counts, nullptr, nullptr, 0, 0};
    hipLaunchKernelGGL(k_geometry, dim3((unsigned)n_contours), dim3(GEOM_TB), 0, ctx->stream, S, d_rows, d_hull);
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

int vpk_contour_geometry_batch(vp_ctx* ctx, const int32_t* d_info, const int32_t* d_counts, const int32_t* d_offsets, const int32_t* d_points, int n,
                               int max_contours, long long max_points, vp_geom_raw* d_rows)
{
    if (n <= 0 || max_contours <= 0) return VP_OK;
    vp_prof_scope ps(ctx, VPK_OTHER);
    geom_src S = {d_points, nullptr, d_counts, d_info, d_offsets, max_contours, max_points};
    hipLaunchKernelGGL(k_geometry, dim3((unsigned)max_contours, (unsigned)n), dim3(GEOM_TB), 0, ctx->stream, S, d_rows, (int32_t*)nullptr);
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
