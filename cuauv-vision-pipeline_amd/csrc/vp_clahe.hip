// cv2.equalizeHist and cv2.createCLAHE(clipLimit, tileGridSize).apply on 8-bit single-channel images (tests/clahe_restate.py is the
// statement; DESIGN.md section 4 has it in words).
//
// equalizeHist: the 256-bin histogram (vpk_hist_u8 for a packed source), one wave that turns it into the 256-byte table
// (k_eq_table), and a table-apply kernel that reads the table from device memory (k_eq_apply).
//
// CLAHE: per tile an integer histogram, cut at the clip limit, the cut amount handed back (clipped / 256 to every bin, the rest one
// each to bins 0, step, 2 step, ...), a prefix sum, one float32 multiply per bin: 256 bytes per tile (k_clahe_hist, and k_clahe_finish
// when several blocks share a tile).  Then every pixel blends the entries of its four nearest tiles' tables with float32 weights
// (k_clahe_apply).  Tiles are cut from the image extended right and down by reflection (BORDER_REFLECT_101) when its size is no
// multiple of the grid; the extension is never stored, the histogram kernel maps the indices while it reads.
//
// Every float32 product and sum below is rounded on its own (__fmul_rn, __fadd_rn, __fsub_rn): a fused multiply-add would change
// results (open points).
#include "vp_internal.h"
#include "vp_clahe_plan.h"
#include <algorithm>

namespace {

static_assert(CL_HIST_BLOCK == 256 && CL_APPLY_BLOCK == 256, "one thread per bin; four waves per block");
static_assert(CL_LDS_BUDGET <= 64 * 1024 && CL_LDS_BUDGET % 16 == 0, "k_clahe_apply: dynamic LDS above 64 KiB");

__device__ __forceinline__ int cl_saturate_u8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Inclusive prefix sum of v over the block's 256 threads in thread order; *total: the sum of all.  sm: 4 words.
__device__ __forceinline__ int cl_scan256(int v, u32* sm, int* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    if (lane == 63) sm[wave] = (u32)v;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int s = (int)sm[k];
        if (k < wave) base += s;
        tot += s;
    }
    __syncthreads();                                     // sm is used again by the next scan
    *total = tot;
    return v + base;
}

// Thread t holds the count of bin t of one tile: clip, redistribute, prefix sum, one multiply -> lut[t].
__device__ __forceinline__ void cl_finish_tile(int v, int clip, float lut_scale, uint8_t* __restrict__ lut, u32* sm)
{
    const int t = threadIdx.x;
    if (clip > 0) {
        const int excess = v > clip ? v - clip : 0;
        v -= excess;
        int clipped;
        (void)cl_scan256(excess, sm, &clipped);          // the block reduction of the excess
        const int batch = clipped >> 8, residual = clipped & 255;
        v += batch;
        if (residual != 0) {                             // bins 0, step, 2 step, ... get one each until `residual` are served
            const int step = 256 / residual;             // >= 1
            if (t % step == 0 && t / step < residual) v++;
        }
    }
    int total;
    const int sum = cl_scan256(v, sm, &total);
    lut[t] = (uint8_t)cl_saturate_u8(__float2int_rn(__fmul_rn((float)sum, lut_scale)));
}

// Histogram of rows [y0, y1) of one tile, columns [x0, x0 + tile_w) of the extended image.  Counters are private to each wave and
// summed at the end.  Source rows are read as dwords at 4-byte aligned addresses wherever a dword lies inside the tile and the row;
// the rest - the tile's ragged ends and the reflected fringe - byte by byte.
// grid (tiles, split), 256 threads.  part == nullptr: this block has the whole tile and finishes its table; otherwise the counts are
// added to part[tile][256] (zeroed by the caller) and k_clahe_finish makes the tables.
__global__ __launch_bounds__(CL_HIST_BLOCK) void k_clahe_hist(const uint8_t* __restrict__ src, size_t sstride, int w, int h, int tiles_x, int tile_w, int tile_h,
                                                              int part_rows, int clip, float lut_scale, u32* __restrict__ part, uint8_t* __restrict__ luts)
{
    __shared__ u32 lh[4 * 256];
    __shared__ u32 sm[4];
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; k++) lh[t + 256 * k] = 0;
    __syncthreads();
    const int tile = blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int x0 = tx * tile_w, x1 = x0 + tile_w;
    const int y0 = ty * tile_h + (int)blockIdx.y * part_rows, y1 = min(ty * tile_h + tile_h, y0 + part_rows);
    const int nslot = (tile_w + 6) / 4;                  // dwords that cover a tile row at every phase
    u32* my = lh + (t >> 6) * 256;
    for (int i = t; i < (y1 - y0) * nslot; i += CL_HIST_BLOCK) {
        const int r = i / nslot, j = i - r * nslot;
        const int ey = y0 + r, sy = ey < h ? ey : 2 * h - 2 - ey;
        const uint8_t* row = src + (size_t)sy * sstride;
        const int ex = x0 - (int)((uintptr_t)(row + x0) & 3u) + 4 * j;       // row + ex is 4-byte aligned
        if (ex >= x1) continue;
        if (ex >= x0 && ex + 4 <= x1 && ex + 4 <= w) {
            const u32 v = *reinterpret_cast<const u32*>(row + ex);
            atomicAdd(&my[v & 255u], 1u);
            atomicAdd(&my[(v >> 8) & 255u], 1u);
            atomicAdd(&my[(v >> 16) & 255u], 1u);
            atomicAdd(&my[v >> 24], 1u);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int e = ex + k;
                if (e >= x0 && e < x1) atomicAdd(&my[row[e < w ? e : 2 * w - 2 - e]], 1u);
            }
        }
    }
    __syncthreads();
    const u32 cnt = lh[t] + lh[t + 256] + lh[t + 512] + lh[t + 768];
    if (part) {
        if (cnt) atomicAdd(part + (size_t)tile * 256 + t, cnt);
        return;
    }
    cl_finish_tile((int)cnt, clip, lut_scale, luts + (size_t)tile * 256, sm);
}

// grid (tiles), 256 threads
__global__ __launch_bounds__(CL_HIST_BLOCK) void k_clahe_finish(const u32* __restrict__ part, int clip, float lut_scale, uint8_t* __restrict__ luts)
{
    __shared__ u32 sm[4];
    cl_finish_tile((int)part[(size_t)blockIdx.x * 256 + threadIdx.x], clip, lut_scale, luts + (size_t)blockIdx.x * 256, sm);
}

// Bytes x .. x + 3 of a row of w bytes (those past the row read as 0), from dwords at 4-byte aligned addresses wherever they lie
// inside the row, whatever the row's own address is.
__device__ __forceinline__ u32 cl_load4(const uint8_t* __restrict__ row, int x, int w)
{
    const uint8_t* p = row + x;
    const int s = (int)((uintptr_t)p & 3u);
    if (x + 4 <= w) {
        if (s == 0) return *reinterpret_cast<const u32*>(p);
        if (x - s >= 0 && x - s + 8 <= w) {
            const u32 lo = *reinterpret_cast<const u32*>(p - s), hi = *reinterpret_cast<const u32*>(p - s + 4);
            return (u32)((((u64)hi << 32) | lo) >> (8 * s));
        }
    }
    u32 v = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (x + k < w) v |= (u32)row[x + k] << (8 * k);
    return v;
}

// result bytes x .. x + 3 of packed row y: one dword where rows keep dwords aligned
__device__ __forceinline__ void cl_store4(uint8_t* __restrict__ dst, int w, int y, int x, u32 out, bool wide)
{
    uint8_t* d = dst + (size_t)y * w + x;
    if (wide) {
        *reinterpret_cast<u32*>(d) = out;
    } else {
        for (int k = 0; k < 4 && x + k < w; k++) d[k] = (uint8_t)(out >> (8 * k));
    }
}

// Tile index and weight along one axis for coordinate p: OpenCV's float32 steps, the clamps after the weights.
__device__ __forceinline__ void cl_axis(int p, float inv_size, int tiles, int* i1, int* i2, float* a, float* a1)
{
    const float f = __fsub_rn(__fmul_rn((float)p, inv_size), 0.5f);
    const int lo = (int)floorf(f);
    *a = __fsub_rn(f, (float)lo);
    *a1 = __fsub_rn(1.f, *a);
    *i1 = max(lo, 0);
    *i2 = min(lo + 1, tiles - 1);
}

// grid (ceil(h / CL_APPLY_ROWS)), 256 threads, four result bytes per lane and turn.  LDS: all tile tables are staged in dynamic LDS
// (tiles * 256 bytes); otherwise they are read where they are.
template <bool LDS>
__global__ __launch_bounds__(CL_APPLY_BLOCK) void k_clahe_apply(const uint8_t* __restrict__ src, size_t sstride, int w, int h, int tiles_x, int tiles_y, int tile_w,
                                                                int tile_h, const uint8_t* __restrict__ luts, uint8_t* __restrict__ dst)
{
    extern __shared__ uint4 cl_tabs[];
    const int t = threadIdx.x;
    const uint8_t* tabs = luts;
    if constexpr (LDS) {
        const int n16 = tiles_x * tiles_y * 16;
        for (int i = t; i < n16; i += CL_APPLY_BLOCK) cl_tabs[i] = reinterpret_cast<const uint4*>(luts)[i];
        __syncthreads();
        tabs = reinterpret_cast<const uint8_t*>(cl_tabs);
    }
    const float inv_tw = __fdiv_rn(1.f, (float)tile_w), inv_th = __fdiv_rn(1.f, (float)tile_h);
    const int y0 = blockIdx.x * CL_APPLY_ROWS, nrows = min(CL_APPLY_ROWS, h - y0), nq = (w + 3) / 4;
    const bool aligned = (((uintptr_t)dst | (uintptr_t)w) & 3u) == 0;
    for (int i = t; i < nrows * nq; i += CL_APPLY_BLOCK) {
        const int r = i / nq, x = 4 * (i - r * nq), y = y0 + r;
        int ty1, ty2;
        float ya, ya1;
        cl_axis(y, inv_th, tiles_y, &ty1, &ty2, &ya, &ya1);
        const uint8_t* plane1 = tabs + (size_t)ty1 * tiles_x * 256;
        const uint8_t* plane2 = tabs + (size_t)ty2 * tiles_x * 256;
        const u32 pix = cl_load4(src + (size_t)y * sstride, x, w);
        u32 out = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (x + k < w) {
                int tx1, tx2;
                float xa, xa1;
                cl_axis(x + k, inv_tw, tiles_x, &tx1, &tx2, &xa, &xa1);
                const int v = (pix >> (8 * k)) & 255u;
                const int o1 = tx1 * 256 + v, o2 = tx2 * 256 + v;
                const float top = __fadd_rn(__fmul_rn((float)plane1[o1], xa1), __fmul_rn((float)plane1[o2], xa));
                const float bot = __fadd_rn(__fmul_rn((float)plane2[o1], xa1), __fmul_rn((float)plane2[o2], xa));
                const float res = __fadd_rn(__fmul_rn(top, ya1), __fmul_rn(bot, ya));
                out |= (u32)cl_saturate_u8(__float2int_rn(res)) << (8 * k);
            }
        }
        cl_store4(dst, w, y, x, out, aligned && x + 4 <= w);
    }
}

// ---- equalizeHist ------------------------------------------------------------------------------------------------------------------------
// One wave, lane l has bins 4 l .. 4 l + 3.  i0: the first non-zero bin.  Every pixel in it: the table holds i0 everywhere.  Otherwise
// scale = float32(255) / float32(total - hist[i0]), lut[i] = saturate(rint(float32(hist[i0 + 1] + .. + hist[i]) * scale)) above i0, 0 up to it.
__global__ __launch_bounds__(64) void k_eq_table(const u32* __restrict__ hist, u32 total, u32* __restrict__ lut32)
{
    const int lane = threadIdx.x;
    u32 c[4];
    int first = 256;
#pragma unroll
    for (int k = 3; k >= 0; k--) {
        c[k] = hist[4 * lane + k];
        if (c[k]) first = 4 * lane + k;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) first = min(first, __shfl_xor(first, d, 64));
    if (first > 255) first = 0;                          // (an empty histogram: the caller never passes one)
    const u32 at0 = hist[first];
    if (at0 == total) {
        lut32[lane] = (u32)first * 0x01010101u;
        return;
    }
    const float scale = __fdiv_rn(255.f, (float)(total - at0));
    int run = 0, incl[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (4 * lane + k > first) run += (int)c[k];
        incl[k] = run;
    }
    int pre = run;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(pre, d, 64);
        if (lane >= d) pre += o;
    }
    pre -= run;                                          // the bins of the lanes before this one
    u32 out = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (4 * lane + k > first) out |= (u32)cl_saturate_u8(__float2int_rn(__fmul_rn((float)(pre + incl[k]), scale))) << (8 * k);
    lut32[lane] = out;
}

// dst = lut[src], the 256-byte table read from device memory; geometry and row access of k_clahe_apply
__global__ __launch_bounds__(CL_APPLY_BLOCK) void k_eq_apply(const uint8_t* __restrict__ src, size_t sstride, int w, int h, const u32* __restrict__ lut32,
                                                             uint8_t* __restrict__ dst)
{
    __shared__ u32 tab32[64];
    const int t = threadIdx.x;
    if (t < 64) tab32[t] = lut32[t];
    __syncthreads();
    const uint8_t* tab = reinterpret_cast<const uint8_t*>(tab32);
    const int y0 = blockIdx.x * CL_APPLY_ROWS, nrows = min(CL_APPLY_ROWS, h - y0), nq = (w + 3) / 4;
    const bool aligned = (((uintptr_t)dst | (uintptr_t)w) & 3u) == 0;
    for (int i = t; i < nrows * nq; i += CL_APPLY_BLOCK) {
        const int r = i / nq, x = 4 * (i - r * nq), y = y0 + r;
        const u32 pix = cl_load4(src + (size_t)y * sstride, x, w);
        const u32 out = (u32)tab[pix & 255u] | (u32)tab[(pix >> 8) & 255u] << 8 | (u32)tab[(pix >> 16) & 255u] << 16 | (u32)tab[pix >> 24] << 24;
        cl_store4(dst, w, y, x, out, aligned && x + 4 <= w);
    }
}

}  // namespace

// sstride: bytes between source rows; d_part: tiles * 256 counters, needed when P.split > 1; d_luts: tiles * 256 bytes, 16-byte aligned
int vpk_clahe(vp_ctx* ctx, const uint8_t* d_src, size_t sstride, int w, int h, int tiles_x, int tiles_y, const vp_clahe_plan& P, u32* d_part, uint8_t* d_luts,
              uint8_t* d_dst)
{
    vp_prof_scope ps(ctx, VPK_OTHER);
    const int tiles = tiles_x * tiles_y;
    if (P.split > 1) {
        VP_HIP(ctx, hipMemsetAsync(d_part, 0, (size_t)tiles * 1024, ctx->stream));
        hipLaunchKernelGGL(k_clahe_hist, dim3(P.hist_gx, P.hist_gy), dim3(CL_HIST_BLOCK), 0, ctx->stream, d_src, sstride, w, h, tiles_x, P.tile_w, P.tile_h, P.part_rows,
                           P.clip, P.lut_scale, d_part, d_luts);
        hipLaunchKernelGGL(k_clahe_finish, dim3(P.hist_gx), dim3(CL_HIST_BLOCK), 0, ctx->stream, d_part, P.clip, P.lut_scale, d_luts);
    } else {
        hipLaunchKernelGGL(k_clahe_hist, dim3(P.hist_gx, 1), dim3(CL_HIST_BLOCK), 0, ctx->stream, d_src, sstride, w, h, tiles_x, P.tile_w, P.tile_h, P.tile_h, P.clip,
                           P.lut_scale, (u32*)nullptr, d_luts);
    }
    VP_HIP(ctx, hipGetLastError());
    if (P.tables_in_lds)
        hipLaunchKernelGGL(k_clahe_apply<true>, dim3(P.apply_gx), dim3(CL_APPLY_BLOCK), P.lds_bytes, ctx->stream, d_src, sstride, w, h, tiles_x, tiles_y, P.tile_w,
                           P.tile_h, d_luts, d_dst);
    else
        hipLaunchKernelGGL(k_clahe_apply<false>, dim3(P.apply_gx), dim3(CL_APPLY_BLOCK), 0, ctx->stream, d_src, sstride, w, h, tiles_x, tiles_y, P.tile_w, P.tile_h,
                           d_luts, d_dst);
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

// histogram -> table by one wave -> table applied from device memory: three launches, nothing comes back.  d_hist: 256 counters;
// d_lut: 256 bytes, 4-byte aligned.  A packed source goes through the histogram kernel of the Otsu family; one with a row stride is
// counted by k_clahe_hist as a single tile shared by many blocks.
int vpk_equalize_hist(vp_ctx* ctx, const uint8_t* d_src, size_t sstride, int w, int h, u32* d_hist, uint8_t* d_lut, uint8_t* d_dst)
{
    if (sstride == (size_t)w) {
        const int rc = vpk_hist_u8(ctx, d_src, (size_t)w * h, d_hist);
        if (rc != VP_OK) return rc;
    } else {
        VP_HIP(ctx, hipMemsetAsync(d_hist, 0, 1024, ctx->stream));
        const int parts = std::max(1, std::min(h, ctx->num_cu * 4)), part_rows = (h + parts - 1) / parts;
        hipLaunchKernelGGL(k_clahe_hist, dim3(1, (unsigned)((h + part_rows - 1) / part_rows)), dim3(CL_HIST_BLOCK), 0, ctx->stream, d_src, sstride, w, h, 1, w, h,
                           part_rows, 0, 0.f, d_hist, (uint8_t*)nullptr);
        VP_HIP(ctx, hipGetLastError());
    }
    vp_prof_scope ps(ctx, VPK_OTHER);
    hipLaunchKernelGGL(k_eq_table, dim3(1), dim3(64), 0, ctx->stream, d_hist, (u32)((size_t)w * h), reinterpret_cast<u32*>(d_lut));
    hipLaunchKernelGGL(k_eq_apply, dim3((unsigned)((h + CL_APPLY_ROWS - 1) / CL_APPLY_ROWS)), dim3(CL_APPLY_BLOCK), 0, ctx->stream, d_src, sstride, w, h,
                       reinterpret_cast<const u32*>(d_lut), d_dst);
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
