// Speckle filter of an int16 disparity image and surface normals of a depth image (tests/speckle_restate.py
// and tests/normals_restate.py are the statements; checks, tile geometry and the normal's formula: vp_speckle_plan.h).
//   k_speckle_local   a block labels one tile in LDS by label equivalence (a pixel's label is the smallest pixel index of its region
//                     inside the tile), counts the pixels of every tile-local region in LDS, and writes per pixel the global index of
//                     its tile-local root and, at the root's own pixel, the count (0 everywhere else)
//   k_speckle_merge   one wave per tile: links across the tile's right and bottom edge, unions on the global label image
//   k_speckle_roots   every tile-local root finds its final root, points at it, and adds its count to the final root's: one device
//                     atomic per tile-local region, none per pixel
//   k_speckle_write   pixel -> tile-local root -> final root -> count; regions at or below the limit become new_val
// Every loop ends on its own progress: a label only ever decreases and never below 0, a find walks strictly down, and a union's larger
// root strictly decreases from one round to the next.  Nothing waits for another block; what needs the whole image is the next launch.
//   k_normals         one thread per pixel, the five depths of the cross stencil, IEEE double without contraction
#include "vp_internal.h"
#include "vp_speckle_plan.h"

#define SP_N (SP_TILE * SP_TILE)
#define SP_ROW_THREADS (SP_TILE / SP_QUAD)

// up to four int16 of a row from p (n of them inside the image, 1..4) as one quad, two pairs or scalars, whichever p's alignment allows
__device__ __forceinline__ void sp_load4(const int16_t* p, int n, int v[4])
{
    if (n == 4 && ((uintptr_t)p & 7) == 0) {
        const uint2 q = *(const uint2*)p;
        v[0] = (int16_t)(q.x & 0xffffu); v[1] = (int16_t)(q.x >> 16); v[2] = (int16_t)(q.y & 0xffffu); v[3] = (int16_t)(q.y >> 16);
    } else if (n == 4 && ((uintptr_t)p & 3) == 0) {
        const u32 a = *(const u32*)p, b = *(const u32*)(p + 2);
        v[0] = (int16_t)(a & 0xffffu); v[1] = (int16_t)(a >> 16); v[2] = (int16_t)(b & 0xffffu); v[3] = (int16_t)(b >> 16);
    } else {
        for (int k = 0; k < 4; k++) v[k] = k < n ? (int)p[k] : 0;
    }
}

__device__ __forceinline__ void sp_store4(int16_t* p, int n, const int v[4])
{
    const u32 a = ((u32)v[0] & 0xffffu) | ((u32)v[1] << 16), b = ((u32)v[2] & 0xffffu) | ((u32)v[3] << 16);
    if (n == 4 && ((uintptr_t)p & 7) == 0) *(uint2*)p = make_uint2(a, b);
    else if (n == 4 && ((uintptr_t)p & 3) == 0) { *(u32*)p = a; *(u32*)(p + 2) = b; }
    else
        for (int k = 0; k < n; k++) p[k] = (int16_t)v[k];
}

// ---- label equivalence in LDS ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ int sp_find_lds(const volatile int* L, int a)
{
    for (int p = L[a]; p != a; p = L[a]) a = p;         // L[a] <= a: strictly down, at most a steps
    return a;
}

__device__ __forceinline__ void sp_union_lds(int* L, int a, int b)
{
    for (;;) {
        a = sp_find_lds(L, a);
        b = sp_find_lds(L, b);
        if (a == b) return;
        if (a > b) { const int s = a; a = b; b = s; }
        const int old = atomicMin(&L[b], a);             // b was a root when found; if it no longer is, go on from what it pointed at
        if (old == b) return;
        b = old;                                         // old < b: the larger side strictly decreases
    }
}

__global__ __launch_bounds__(SP_THREADS) void k_speckle_local(const int16_t* __restrict__ src, size_t sstride, int w, int h, int new_val, int max_diff, int lpitch,
                                                              int* __restrict__ label, int* __restrict__ count)
{
    __shared__ int L[SP_N];          // label: a pixel index of the tile, -1 for a pixel of no region (new_val, or outside the image)
    __shared__ int V[SP_N];          // value
    __shared__ int Cn[SP_N];         // pixels of the region whose root this is
    const int t = threadIdx.x, ty = t / SP_ROW_THREADS, tx = (t % SP_ROW_THREADS) * SP_QUAD, i0 = ty * SP_TILE + tx;
    const int gx = (int)blockIdx.x * SP_TILE + tx, gy = (int)blockIdx.y * SP_TILE + ty;
    const int n_in = gy < h ? min(SP_QUAD, max(0, w - gx)) : 0;
    int v[4] = {0, 0, 0, 0}, lab[4], r[4];
    bool ok[4];
    if (n_in > 0) sp_load4((const int16_t*)((const uint8_t*)src + (size_t)gy * sstride) + gx, n_in, v);
    for (int k = 0; k < 4; k++) {
        ok[k] = k < n_in && v[k] != new_val;
        lab[k] = !ok[k] ? -1 : (k > 0 && ok[k - 1] && vp_speckle_linked(v[k - 1], v[k], max_diff)) ? lab[k - 1] : i0 + k;   // runs inside the quad
        L[i0 + k] = lab[k];
        V[i0 + k] = v[k];
        Cn[i0 + k] = 0;
    }
    __syncthreads();
    const volatile int* Lr = L;
    if (tx > 0 && ok[0] && Lr[i0 - 1] >= 0 && vp_speckle_linked(V[i0 - 1], v[0], max_diff)) sp_union_lds(L, i0, i0 - 1);
    if (ty > 0) {
        bool prev = false;
        for (int k = 0; k < 4; k++) {
            const int up = i0 + k - SP_TILE;
            const bool link = ok[k] && Lr[up] >= 0 && vp_speckle_linked(V[up], v[k], max_diff);
            // the pixel to the left is in this run and linked upwards, and the two pixels above are linked: nothing new to say
            const bool known = link && prev && lab[k] == lab[k - 1] && vp_speckle_linked(V[up - 1], V[up], max_diff);
            if (link && !known) sp_union_lds(L, i0 + k, up);
            prev = link;
        }
    }
    __syncthreads();
    for (int k = 0; k < 4; k++) r[k] = ok[k] ? sp_find_lds(L, i0 + k) : -1;
    // Counting: the lanes of a wave that share the first active lane's root add once between them, the others one each.  A clean
    // image is one region per tile: 64 LDS atomics per tile then, not 1024 on one address.
    const int lane = t & 63;
    for (int k = 0; k < 4; k++) {
        const u64 active = __ballot(ok[k]);
        const int first = active ? __ffsll((long long)active) - 1 : 0;
        const int lead = __shfl(r[k], first);
        const bool same = ok[k] && r[k] == lead;
        const u64 sharing = __ballot(same);
        if (same) {
            if (lane == first) atomicAdd(&Cn[lead], __popcll(sharing));
        } else if (ok[k]) atomicAdd(&Cn[r[k]], 1);
    }
    __syncthreads();
    if (gy < h && gx < lpitch) {                        // lpitch is a whole number of quads: the quad lies inside the two images' rows
        const int base = (int)blockIdx.y * SP_TILE * lpitch + (int)blockIdx.x * SP_TILE;
        int gl[4], gc[4];
        for (int k = 0; k < 4; k++) {
            gl[k] = ok[k] ? base + (r[k] / SP_TILE) * lpitch + r[k] % SP_TILE : -1;
            gc[k] = ok[k] && r[k] == i0 + k ? Cn[i0 + k] : 0;
        }
        const size_t at = (size_t)gy * lpitch + gx;
        *(int4*)(label + at) = make_int4(gl[0], gl[1], gl[2], gl[3]);
        *(int4*)(count + at) = make_int4(gc[0], gc[1], gc[2], gc[3]);
    }
}

// ---- unions on the global label image ----------------------------------------------------------------------------------------------
// Labels change under other blocks' atomics while this one reads them: the reads go to the device's coherence point, and whatever
// they return is a label the entry held at some time, which is a pixel of the same region with an index no larger.
__device__ __forceinline__ int sp_label_load(const int* label, int a) { return __hip_atomic_load(label + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int sp_find_dev(const int* label, int a)
{
    for (int p = sp_label_load(label, a); p != a; p = sp_label_load(label, a)) a = p;
    return a;
}

__device__ __forceinline__ void sp_union_dev(int* label, int a, int b)
{
    for (;;) {
        a = sp_find_dev(label, a);
        b = sp_find_dev(label, b);
        if (a == b) return;
        if (a > b) { const int s = a; a = b; b = s; }
        const int old = atomicMin(label + b, a);
        if (old == b) return;
        b = old;
    }
}

__global__ __launch_bounds__(64) void k_speckle_merge(const int16_t* __restrict__ src, size_t sstride, int w, int h, int new_val, int max_diff, int lpitch, int* label)
{
    // lanes 0..31: the tile's right edge against the next tile's left column; lanes 32..63: its bottom edge against the row below
    const int t = threadIdx.x, j = t & (SP_TILE - 1);
    const bool below = t >= SP_TILE;
    const int x = (int)blockIdx.x * SP_TILE + (below ? j : SP_TILE - 1), y = (int)blockIdx.y * SP_TILE + (below ? SP_TILE - 1 : j);
    const int nx = below ? x : x + 1, ny = below ? y + 1 : y;
    int a = new_val, b = new_val;
    if (nx < w && ny < h) {
        a = *((const int16_t*)((const uint8_t*)src + (size_t)y * sstride) + x);
        b = *((const int16_t*)((const uint8_t*)src + (size_t)ny * sstride) + nx);
    }
    const bool link = a != new_val && b != new_val && vp_speckle_linked(a, b, max_diff);
    // the pair before this one on the same edge is linked, and both sides run on into this pair: that union says it all
    const int pa = __shfl_up(a, 1), pb = __shfl_up(b, 1);
    const bool plink = __shfl_up((int)link, 1) != 0;
    const bool known = j > 0 && link && plink && vp_speckle_linked(pa, a, max_diff) && vp_speckle_linked(pb, b, max_diff);
    if (link && !known) sp_union_dev(label, y * lpitch + x, ny * lpitch + nx);
}

__global__ __launch_bounds__(256) void k_speckle_roots(int n_quads, int* label, int* count)
{
    const int q = (int)blockIdx.x * 256 + threadIdx.x;
    if (q >= n_quads) return;
    // a count above 0 marks a tile-local root.  A final root's own count is being added to meanwhile, but a final root does not use
    // what it read; every other entry is only ever written by the launch before.
    const int4 c4 = *(const int4*)(count + (size_t)q * 4);
    const int c[4] = {c4.x, c4.y, c4.z, c4.w};
    for (int k = 0; k < 4; k++) {
        if (c[k] <= 0) continue;
        const int p = q * 4 + k, root = sp_find_dev(label, p);
        if (root == p) continue;
        __hip_atomic_store(label + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        atomicAdd(count + root, c[k]);                  // at most w * h in all: no overflow
    }
}

__global__ __launch_bounds__(256) void k_speckle_write(const int16_t* src, size_t sstride, int w, int h, int new_val, int max_size, int lpitch,
                                                       const int* __restrict__ label, const int* __restrict__ count, int16_t* dst, size_t dstride)
{
    const int gx = ((int)blockIdx.x * 256 + threadIdx.x) * SP_QUAD, y = blockIdx.y;
    if (gx >= w) return;
    const int n_in = min(SP_QUAD, w - gx);
    int v[4];
    sp_load4((const int16_t*)((const uint8_t*)src + (size_t)y * sstride) + gx, n_in, v);
    if (label) {                                        // (uniform) NULL: a plain copy, max_speckle_size 0
        const int4 l4 = *(const int4*)(label + (size_t)y * lpitch + gx);
        const int l[4] = {l4.x, l4.y, l4.z, l4.w};
        int last = -1;
        bool keep = true;
        for (int k = 0; k < n_in; k++) {
            if (l[k] < 0) continue;
            if (l[k] != last) {
                last = l[k];
                keep = count[label[last]] > max_size;   // a tile-local root points at its final root, a final root at itself
            }
            if (!keep) v[k] = new_val;
        }
    }
    sp_store4((int16_t*)((uint8_t*)dst + (size_t)y * dstride) + gx, n_in, v);
}

int vpk_filter_speckles(vp_ctx* ctx, const int16_t* d_src, size_t sstride, int w, int h, int new_val, int max_size, int max_diff, const vp_speckle_plan& P, uint8_t* d_ws,
                        int16_t* d_dst, size_t dstride)
{
    const dim3 wgrid((unsigned)((P.lpitch / SP_QUAD + 255) / 256), (unsigned)h);
    if (max_size == 0) {
        if (d_dst == d_src) return VP_OK;
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_speckle_write, wgrid, dim3(256), 0, ctx->stream, d_src, sstride, w, h, new_val, 0, P.lpitch, (const int*)nullptr, (const int*)nullptr, d_dst,
                           dstride);
        VP_HIP(ctx, hipGetLastError());
        return VP_OK;
    }
    int *label = (int*)d_ws, *count = (int*)(d_ws + P.off_count);
    const int n_quads = P.lpitch / SP_QUAD * h;
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_speckle_local, dim3(P.grid_x, P.grid_y), dim3(SP_THREADS), 0, ctx->stream, d_src, sstride, w, h, new_val, max_diff, P.lpitch, label, count);
    }
    VP_HIP(ctx, hipGetLastError());
    if (P.grid_x > 1 || P.grid_y > 1) {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_speckle_merge, dim3(P.grid_x, P.grid_y), dim3(64), 0, ctx->stream, d_src, sstride, w, h, new_val, max_diff, P.lpitch, label);
        VP_HIP(ctx, hipGetLastError());
    }
    if (P.grid_x > 1 || P.grid_y > 1) {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_speckle_roots, dim3((unsigned)((n_quads + 255) / 256)), dim3(256), 0, ctx->stream, n_quads, label, count);
        VP_HIP(ctx, hipGetLastError());
    }
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_speckle_write, wgrid, dim3(256), 0, ctx->stream, d_src, sstride, w, h, new_val, max_size, P.lpitch, (const int*)label, (const int*)count, d_dst,
                           dstride);
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

// ---- surface normals ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_normals(const float* __restrict__ depth, size_t zpitch, int w, int h, double f, double cx, double cy, double jump, int encode,
                                                 float* __restrict__ normals, size_t npitch)
{
    const int x = (int)blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    float n[3] = {0.0f, 0.0f, 0.0f};
    bool have = false;
    if (x >= 1 && y >= 1 && x <= w - 2 && y <= h - 2) {
        const float* z = depth + (size_t)y * zpitch + x;
        have = vp_normal_at(x, y, z[0], z[-1], z[1], z[-(ptrdiff_t)zpitch], z[zpitch], f, cx, cy, jump, n);
    }
    vp_normal_store(have, n, encode, normals + (size_t)y * npitch + (size_t)x * 3);
}

int vpk_normals(vp_ctx* ctx, const float* d_depth, size_t zstride, int w, int h, double f, double cx, double cy, double jump, int encode, float* d_normals, size_t nstride)
{
    vp_prof_scope ps(ctx, VPK_OTHER);
    hipLaunchKernelGGL(k_normals, dim3((unsigned)((w + 255) / 256), (unsigned)h), dim3(256), 0, ctx->stream, d_depth, zstride / 4, w, h, f, cx, cy, jump, encode, d_normals,
                       nstride / 4);
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
