// Colour-histogram tracking on uint8 images (the statement: tests/hist_restate.py; checks, bin tables, limits
// and grids: vp_hist_plan.h): cv2.calcHist as exact uint32 counts, cv2.calcBackProject as a gather from a folded byte table, and
// cv2.meanShift with its whole loop inside one block per window.  Everything is integer arithmetic except mean shift's two divisions,
// which are explicit round-to-nearest double intrinsics on exact integers.
#include "vp_internal.h"
#include "vp_hist_plan.h"

// The three tables as premultiplied offsets in LDS: the counter (table entry) of a pixel is the sum of its three lookups, negative
// when a channel falls into no bin.  An unused dimension has a table of zeros.
__device__ __forceinline__ void hs_stage_tabs(const vp_hist_tabs& T, int step0, int step1, int step2, int* s_tab)
{
    for (int i = threadIdx.x; i < HS_MAX_DIMS * 256; i += HS_THREADS) {
        const int d = i >> 8, b = T.bin[i];
        s_tab[i] = b == HS_OUT_BIN ? HS_OUT_OFFSET : b * (d == 0 ? step0 : d == 1 ? step1 : step2);
    }
}

// HS_PX neighbouring pixels of a row, whole words when the row allows it
template <int CN>
__device__ __forceinline__ void hs_load(const uint8_t* row, int npx, uint8_t* out)
{
    if (npx == HS_PX && ((uintptr_t)row & 3) == 0) {
#pragma unroll
        for (int i = 0; i < CN; i++) reinterpret_cast<u32*>(out)[i] = reinterpret_cast<const u32*>(row)[i];
    } else {
#pragma unroll
        for (int i = 0; i < HS_PX * CN; i++) out[i] = i < npx * CN ? row[i] : (uint8_t)0;
    }
}

// Counts into `hist` (zeroed before the launch).  A lane takes HS_PX neighbouring pixels at a time and keeps the length of its
// current run of equal bins in a register; a pixel of another bin sends the run to the counters with one atomic.  What the lanes
// still hold at the end goes in one of two ways: when a ballot shows one bin for the whole wave - a uniform image -, the lengths are
// added across the wave and one lane adds the sum; otherwise every lane adds its own.  IN_LDS: the counters are the block's private
// copy in LDS, flushed to device memory once per block (non-zero counters only); otherwise they are the device counters themselves.
template <int CN, bool IN_LDS>
__global__ __launch_bounds__(HS_THREADS) void k_calc_hist(const uint8_t* __restrict__ src, size_t stride, int w, int h, vp_hist_tabs T, int c0, int c1, int c2,
                                                           int step0, int step1, int step2, int total, const uint8_t* __restrict__ mask, size_t mstride,
                                                           const u64* __restrict__ mbits, u32* __restrict__ hist)
{
    extern __shared__ __align__(16) u32 hs_lds[];
    int* s_tab = reinterpret_cast<int*>(hs_lds);
    u32* s_cnt = hs_lds + HS_MAX_DIMS * 256;
    const int tid = threadIdx.x;
    hs_stage_tabs(T, step0, step1, step2, s_tab);
    if (IN_LDS)
        for (int i = tid; i < total; i += HS_THREADS) s_cnt[i] = 0;
    __syncthreads();
    u32* cnt = IN_LDS ? s_cnt : hist;

    const u32 cpr = (u32)(w + HS_PX - 1) / HS_PX, chunks = cpr * (u32)h, wpr = (u32)(w + 63) / 64;
    int cur = -1;
    u32 rn = 0;
    for (u32 c = blockIdx.x * HS_THREADS + (u32)tid; c < chunks; c += gridDim.x * HS_THREADS) {
        const u32 y = c / cpr, x0 = (c - y * cpr) * HS_PX;
        const int npx = (int)(w - x0) < HS_PX ? (int)(w - x0) : HS_PX;
        u32 on = 0xf;
        if (mbits) on = (u32)(mbits[(size_t)y * wpr + x0 / 64] >> (x0 & 63)) & 0xf;   // x0 is a multiple of 4: the four bits share a word
        else if (mask) {
            const uint8_t* m = mask + (size_t)y * mstride + x0;
            on = 0;
#pragma unroll
            for (int j = 0; j < HS_PX; j++)
                if (j < npx && m[j]) on |= 1u << j;
        }
        if (!on) continue;
        __align__(4) uint8_t px[HS_PX * CN];
        hs_load<CN>(src + (size_t)y * stride + (size_t)x0 * CN, npx, px);
#pragma unroll
        for (int j = 0; j < HS_PX; j++) {
            if (j >= npx) break;
            const int idx = s_tab[px[j * CN + c0]] + s_tab[256 + px[j * CN + c1]] + s_tab[512 + px[j * CN + c2]];
            if (idx < 0 || !((on >> j) & 1)) continue;
            if (idx != cur) {
                if (rn) atomicAdd(&cnt[cur], rn);
                cur = idx;
                rn = 0;
            }
            rn++;
        }
    }
    // every lane of the wave is here (none has returned), so the ballots see all 64
    const u64 holders = __ballot(rn != 0);
    if (holders) {
        const int first = __ffsll((long long)holders) - 1;
        const int bin0 = __shfl(cur, first, 64);
        if (__ballot(rn != 0 && cur != bin0) == 0) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) rn += __shfl_xor(rn, m, 64);
            if ((tid & 63) == 0) atomicAdd(&cnt[bin0], rn);
        } else if (rn) atomicAdd(&cnt[cur], rn);
    }
    if (IN_LDS) {
        __syncthreads();
        for (int i = tid; i < total; i += HS_THREADS)
            if (s_cnt[i]) atomicAdd(&hist[i], s_cnt[i]);
    }
}

// table[i] = saturate_u8(round_half_even(double(hist[i]) * scale)); a NaN gives 0
__global__ __launch_bounds__(256) void k_bp_fold(const float* __restrict__ hist, int total, double scale, uint8_t* __restrict__ table)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const double r = rint(__dmul_rn((double)hist[i], scale));
    table[i] = !(r > 0.0) ? (uint8_t)0 : r >= 255.0 ? (uint8_t)255 : (uint8_t)(int)r;
}

// dst = table[bin of the pixel], 0 for a pixel without a bin.  IN_LDS: the block reads the table from its own copy in LDS.
template <int CN, bool IN_LDS>
__global__ __launch_bounds__(HS_THREADS) void k_back_project(const uint8_t* __restrict__ src, size_t stride, int w, int h, vp_hist_tabs T, int c0, int c1, int c2,
                                                              int step0, int step1, int step2, int total, const uint8_t* __restrict__ table,
                                                              uint8_t* __restrict__ dst, size_t dstride)
{
    extern __shared__ __align__(16) u32 hs_lds[];
    int* s_tab = reinterpret_cast<int*>(hs_lds);
    uint8_t* s_bytes = reinterpret_cast<uint8_t*>(hs_lds + HS_MAX_DIMS * 256);
    const int tid = threadIdx.x;
    hs_stage_tabs(T, step0, step1, step2, s_tab);
    if (IN_LDS) {
        if (((uintptr_t)table & 3) == 0) {
            const int words = total / 4;
            for (int i = tid; i < words; i += HS_THREADS) reinterpret_cast<u32*>(s_bytes)[i] = reinterpret_cast<const u32*>(table)[i];
            for (int i = words * 4 + tid; i < total; i += HS_THREADS) s_bytes[i] = table[i];
        } else
            for (int i = tid; i < total; i += HS_THREADS) s_bytes[i] = table[i];
    }
    __syncthreads();
    const uint8_t* tab = IN_LDS ? s_bytes : table;

    const u32 cpr = (u32)(w + HS_PX - 1) / HS_PX, chunks = cpr * (u32)h;
    for (u32 c = blockIdx.x * HS_THREADS + (u32)tid; c < chunks; c += gridDim.x * HS_THREADS) {
        const u32 y = c / cpr, x0 = (c - y * cpr) * HS_PX;
        const int npx = (int)(w - x0) < HS_PX ? (int)(w - x0) : HS_PX;
        __align__(4) uint8_t px[HS_PX * CN];
        hs_load<CN>(src + (size_t)y * stride + (size_t)x0 * CN, npx, px);
        uint8_t r[HS_PX];
#pragma unroll
        for (int j = 0; j < HS_PX; j++) {
            const int idx = s_tab[px[j * CN + c0]] + s_tab[256 + px[j * CN + c1]] + s_tab[512 + px[j * CN + c2]];
            r[j] = (j < npx && idx >= 0) ? tab[idx] : (uint8_t)0;
        }
        uint8_t* out = dst + (size_t)y * dstride + x0;
        if (npx == HS_PX && ((uintptr_t)out & 3) == 0)
            *reinterpret_cast<u32*>(out) = (u32)r[0] | (u32)r[1] << 8 | (u32)r[2] << 16 | (u32)r[3] << 24;
        else {
#pragma unroll
            for (int j = 0; j < HS_PX; j++)
                if (j < npx) out[j] = r[j];
        }
    }
}

// cv2.meanShift, one block per window, the whole loop inside (tests/hist_restate.py mean_shift).  Per iteration the waves take the
// window's rows in turn; a lane sums whole aligned words of a row (and one of the at most six bytes before and after them) into
// 32-bit row sums s0 = sum p and s1 = sum x p, and adds them - s0 weighted by the row for m01 - to 64-bit totals, which are exact
// on a full 4096 x 4096 window of 255s.  The totals are added across the wave, then across the waves through LDS; lane 0 takes the
// step in double and leaves the next window, or the end, in LDS for all.  out: (x, y, w, h, iterations) per window.
__global__ __launch_bounds__(HS_MS_THREADS) void k_mean_shift(const uint8_t* __restrict__ src, size_t stride, int cols, int rows, const int32_t* __restrict__ windows,
                                                               int niters, int eps2, int32_t* __restrict__ out)
{
    __shared__ u64 s_part[HS_MS_THREADS / 64][3];
    __shared__ int s_cur[4];
    __shared__ int s_stop;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t* win = windows + 4 * blockIdx.x;
    // W = window cut to the image (the host has checked that something is left)
    int cx = win[0] > 0 ? win[0] : 0, cy = win[1] > 0 ? win[1] : 0;
    const long long wx1 = (long long)win[0] + win[2], wy1 = (long long)win[1] + win[3];
    int cw = (int)(wx1 < cols ? wx1 : cols) - cx, ch = (int)(wy1 < rows ? wy1 : rows) - cy;
    const double half_w = cw * 0.5, half_h = ch * 0.5;
    int i = 0;
    for (; i < niters; i++) {
        // cur = cur cut to the image; cv2's empty Rect() is re-centred, and a side is at least 1
        {
            const int x0 = cx > 0 ? cx : 0, y0 = cy > 0 ? cy : 0;
            const int x1 = cx + cw < cols ? cx + cw : cols, y1 = cy + ch < rows ? cy + ch : rows;
            if (x1 <= x0 || y1 <= y0) { cx = cols / 2; cy = rows / 2; cw = 0; ch = 0; }
            else { cx = x0; cy = y0; cw = x1 - x0; ch = y1 - y0; }
            if (cw < 1) cw = 1;
            if (ch < 1) ch = 1;
        }
        u64 m00 = 0, m10 = 0, m01 = 0;
        for (int r = wave; r < ch; r += HS_MS_THREADS / 64) {
            const uint8_t* a = src + (size_t)(cy + r) * stride + cx;
            int head = (int)((4 - ((uintptr_t)a & 3)) & 3);
            if (head > cw) head = cw;
            const int nwords = (cw - head) / 4, tail = cw - head - 4 * nwords;
            u32 s0 = 0, s1 = 0;
            for (int wi = lane; wi < nwords; wi += 64) {
                const u32 v = *reinterpret_cast<const u32*>(a + head + 4 * wi);
                const u32 b0 = v & 255, b1 = (v >> 8) & 255, b2 = (v >> 16) & 255, b3 = v >> 24, s = b0 + b1 + b2 + b3;
                s0 += s;
                s1 += (u32)(head + 4 * wi) * s + b1 + 2 * b2 + 3 * b3;
            }
            if (lane < head + tail) {
                const int x = lane < head ? lane : 4 * nwords + lane;      // (head + 4 nwords + (lane - head))
                const u32 p = a[x];
                s0 += p;
                s1 += (u32)x * p;
            }
            m00 += s0;
            m10 += s1;
            m01 += (u64)r * s0;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            m00 += __shfl_xor(m00, m, 64);
            m10 += __shfl_xor(m10, m, 64);
            m01 += __shfl_xor(m01, m, 64);
        }
        if (lane == 0) { s_part[wave][0] = m00; s_part[wave][1] = m10; s_part[wave][2] = m01; }
        __syncthreads();
        if (tid == 0) {
            u64 t00 = 0, t10 = 0, t01 = 0;
            for (int k = 0; k < HS_MS_THREADS / 64; k++) { t00 += s_part[k][0]; t10 += s_part[k][1]; t01 += s_part[k][2]; }
            int stop = 0, nx = cx, ny = cy;
            if (t00 == 0) stop = 1;
            else {
                int dx = (int)rint(__dsub_rn(__ddiv_rn((double)t10, (double)t00), half_w));
                int dy = (int)rint(__dsub_rn(__ddiv_rn((double)t01, (double)t00), half_h));
                nx = cx + dx;
                ny = cy + dy;
                nx = nx > 0 ? nx : 0;
                ny = ny > 0 ? ny : 0;
                nx = nx < cols - cw ? nx : cols - cw;
                ny = ny < rows - ch ? ny : rows - ch;
                dx = nx - cx;
                dy = ny - cy;
                if (dx * dx + dy * dy < eps2) stop = 1;
            }
            s_cur[0] = nx;
            s_cur[1] = ny;
            s_stop = stop;
        }
        __syncthreads();
        cx = s_cur[0];
        cy = s_cur[1];
        const int stop = s_stop;
        __syncthreads();                 // every lane has read the step before lane 0 writes the next one
        if (stop) break;
    }
    if (tid == 0) {
        int32_t* o = out + 5 * blockIdx.x;
        o[0] = cx; o[1] = cy; o[2] = cw; o[3] = ch; o[4] = i;
    }
}

#define HS_LAUNCH(kernel, CNV, ...)                                                                                                   \
    switch (CNV) {                                                                                                                    \
    case 1: hipLaunchKernelGGL((kernel<1, true>), __VA_ARGS__); break;                                                                \
    case 2: hipLaunchKernelGGL((kernel<2, true>), __VA_ARGS__); break;                                                                \
    case 3: hipLaunchKernelGGL((kernel<3, true>), __VA_ARGS__); break;                                                                \
    default: hipLaunchKernelGGL((kernel<4, true>), __VA_ARGS__); break;                                                               \
    }
#define HS_LAUNCH_GLOBAL(kernel, CNV, ...)                                                                                            \
    switch (CNV) {                                                                                                                    \
    case 1: hipLaunchKernelGGL((kernel<1, false>), __VA_ARGS__); break;                                                               \
    case 2: hipLaunchKernelGGL((kernel<2, false>), __VA_ARGS__); break;                                                               \
    case 3: hipLaunchKernelGGL((kernel<3, false>), __VA_ARGS__); break;                                                               \
    default: hipLaunchKernelGGL((kernel<4, false>), __VA_ARGS__); break;                                                              \
    }

// a block's dynamic LDS above the default limit has to be allowed per kernel, once per device
template <typename K>
static int hs_allow_lds(vp_ctx* ctx, K kernel, size_t lds)
{
    if (lds > 65536) VP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)HS_LDS_BYTES));
    return VP_OK;
}

int vpk_calc_hist(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, const vp_hist_plan& P, const uint8_t* d_mask, size_t mstride, const u64* d_mbits,
                  u32* d_hist)
{
    VP_HIP(ctx, hipMemsetAsync(d_hist, 0, (size_t)P.total * 4, ctx->stream));
    const dim3 grid(P.grid), block(HS_THREADS);
    if (P.in_lds && P.lds_bytes > 65536) {
        switch (P.cn) {
        case 1: if (int rc = hs_allow_lds(ctx, k_calc_hist<1, true>, P.lds_bytes)) return rc; break;
        case 2: if (int rc = hs_allow_lds(ctx, k_calc_hist<2, true>, P.lds_bytes)) return rc; break;
        case 3: if (int rc = hs_allow_lds(ctx, k_calc_hist<3, true>, P.lds_bytes)) return rc; break;
        default: if (int rc = hs_allow_lds(ctx, k_calc_hist<4, true>, P.lds_bytes)) return rc; break;
        }
    }
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        if (P.in_lds) {
            HS_LAUNCH(k_calc_hist, P.cn, grid, block, P.lds_bytes, ctx->stream, d_src, stride, w, h, P.tabs, P.channel[0], P.channel[1], P.channel[2], P.step[0],
                      P.step[1], P.step[2], P.total, d_mask, mstride, d_mbits, d_hist)
        } else {
            HS_LAUNCH_GLOBAL(k_calc_hist, P.cn, grid, block, P.lds_bytes, ctx->stream, d_src, stride, w, h, P.tabs, P.channel[0], P.channel[1], P.channel[2], P.step[0],
                             P.step[1], P.step[2], P.total, d_mask, mstride, d_mbits, d_hist)
        }
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

int vpk_back_project_fold(vp_ctx* ctx, const float* d_hist, int total, double scale, uint8_t* d_table)
{
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_bp_fold, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, d_hist, total, scale, d_table);
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

int vpk_back_project(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, const vp_hist_plan& P, const uint8_t* d_table, uint8_t* d_dst, size_t dstride)
{
    const dim3 grid(P.grid), block(HS_THREADS);
    if (P.in_lds && P.lds_bytes > 65536) {
        switch (P.cn) {
        case 1: if (int rc = hs_allow_lds(ctx, k_back_project<1, true>, P.lds_bytes)) return rc; break;
        case 2: if (int rc = hs_allow_lds(ctx, k_back_project<2, true>, P.lds_bytes)) return rc; break;
        case 3: if (int rc = hs_allow_lds(ctx, k_back_project<3, true>, P.lds_bytes)) return rc; break;
        default: if (int rc = hs_allow_lds(ctx, k_back_project<4, true>, P.lds_bytes)) return rc; break;
        }
    }
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        if (P.in_lds) {
            HS_LAUNCH(k_back_project, P.cn, grid, block, P.lds_bytes, ctx->stream, d_src, stride, w, h, P.tabs, P.channel[0], P.channel[1], P.channel[2], P.step[0],
                      P.step[1], P.step[2], P.total, d_table, d_dst, dstride)
        } else {
            HS_LAUNCH_GLOBAL(k_back_project, P.cn, grid, block, P.lds_bytes, ctx->stream, d_src, stride, w, h, P.tabs, P.channel[0], P.channel[1], P.channel[2],
                             P.step[0], P.step[1], P.step[2], P.total, d_table, d_dst, dstride)
        }
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

int vpk_mean_shift(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, const int32_t* d_windows, int n, int niters, int eps2, int32_t* d_out)
{
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_mean_shift, dim3((unsigned)n), dim3(HS_MS_THREADS), 0, ctx->stream, d_src, stride, w, h, d_windows, niters, eps2, d_out);
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
