// White balance in Lab for gfx950: utils/color.py:370-378 `white_balance_bgr` and :381-392 `white_balance_bgr_blur`.
//
// Both take an 8-bit BGR image to Lab (RGB2Lab_b), move a and b by (mean - 128) in float32, cast them back to uint8 the way numpy's
// astype does (truncation toward zero, low 8 bits kept: -1.5 -> 255, 256.2 -> 0) and convert back (Lab2RGBinteger).  The Lab image
// is never stored: the last pass reads BGR again and recomputes it, which costs less HBM traffic than a round trip of 3 B/px.
//
// Global mean (np.mean of the float32 plane): numpy sums a contiguous float32 plane as consecutive 8192-element chunks, each chunk
// pairwise, and adds the chunk sums in order into a float32 accumulator starting at 0; the float32 total is divided by the count in
// binary64 (np.float32 / np.intp) and rounded to float32.  Inside a chunk every partial sum is an integer below 2^24, so a chunk sum is
// exact in any order: k_wb_chunk_sums sums chunks as integers, k_wb_fold adds them in float32 in chunk order (one wave), and
// k_wb_apply reads the two means from device memory - no host round trip.
//
// Box mean (cv2.blur, BORDER_REPLICATE, float32): OpenCV's 32F box filter sums in binary64, exact here (integer sums), and scales by
// the binary64 reciprocal 1.0 / (k k).  Cost per pixel is independent of k: row prefix sums (k_wbb_row_prefix), column prefix sums of
// the clamped row-window sums per 64-row tile (k_wbb_col_prefix) with the tile carries (k_wbb_carry), and the clamped column window as a
// difference of two prefix sums plus the replicated-border counts (k_wbb_apply).  Sums are taken modulo 2^32: a box sum is at most
// k^2 * 255 < 2^32 for k <= VP_WB_MAX_KERNEL, so differences of wrapped prefix sums are exact.
#include "vp_lab.h"
#include <algorithm>

#define WB_CHUNK 8192   // numpy's reduction buffer size
#define WB_TILE 64      // rows per column-prefix tile

struct WbLds { LabLds fwd; LabInvLds inv; };

__device__ __forceinline__ void load_wb_lds(WbLds& s, const vp_tables& tab)
{
    load_lab_lds(s.fwd, tab);
    load_labinv_lds(s.inv, tab);
    __syncthreads();
}

// numpy's float32 -> uint8 astype: truncate toward zero, keep the low 8 bits (the values here lie in [-128, 384))
__device__ __forceinline__ int wrap_u8(float v) { return ((int)v) & 255; }

// one pixel of the second pass: Lab of (b, g, r), a and b moved by the float32 shifts (mean - 128), back to BGR
__device__ __forceinline__ void wb_px(const WbLds& s, const int32_t* __restrict__ abxz, const uint8_t* p, float sa, float sb, uint8_t* q)
{
    int L = 0, A = 0, B = 0;
    lab_px<7>(s.fwd, p[0], p[1], p[2], L, A, B);
    int c0, c1, c2;
    lab2bgr_px(s.inv, abxz, L, wrap_u8(__fsub_rn((float)A, sa)), wrap_u8(__fsub_rn((float)B, sb)), c0, c1, c2);
    q[0] = (uint8_t)c0; q[1] = (uint8_t)c1; q[2] = (uint8_t)c2;
}

// ---- global mean ---------------------------------------------------------------------------------------------------------------------

// block c: exact integer sums of a and b over pixels [c * 8192, (c + 1) * 8192) of the row-major image
__global__ __launch_bounds__(256) void k_wb_chunk_sums(const uint8_t* __restrict__ src, size_t stride, u32 w, u32 npx, vp_tables tab,
                                                       int2* __restrict__ sums)
{
    __shared__ LabLds s;
    __shared__ int part[2][4];
    load_lab_lds(s, tab);
    __syncthreads();
    int sa = 0, sb = 0;
    const u32 base = blockIdx.x * WB_CHUNK;
    for (u32 j = threadIdx.x; j < WB_CHUNK; j += 256) {
        const u32 p = base + j;
        if (p >= npx) break;
        const u32 y = p / w, x = p - y * w;
        const uint8_t* q = src + (size_t)y * stride + 3 * (size_t)x;
        int L, A = 0, B = 0;
        lab_px<6>(s, q[0], q[1], q[2], L, A, B);
        sa += A;
        sb += B;
    }
    for (int o = 32; o > 0; o >>= 1) {
        sa += __shfl_xor(sa, o);
        sb += __shfl_xor(sb, o);
    }
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = sa; part[1][threadIdx.x >> 6] = sb; }
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = make_int2(part[0][0] + part[0][1] + part[0][2] + part[0][3], part[1][0] + part[1][1] + part[1][2] + part[1][3]);
}

// one wave: the chunk sums are staged through LDS, lane 0 folds a and lane 1 folds b in float32, in chunk order
__global__ __launch_bounds__(64) void k_wb_fold(const int2* __restrict__ sums, u32 nchunks, u32 npx, float* __restrict__ mean)
{
    __shared__ int2 buf[2048];
    float acc = 0.0f;
    for (u32 c0 = 0; c0 < nchunks; c0 += 2048) {
        const u32 n = min(2048u, nchunks - c0);
        __syncthreads();
        for (u32 i = threadIdx.x; i < n; i += 64) buf[i] = sums[c0 + i];
        __syncthreads();
        if (threadIdx.x < 2) {
#pragma unroll 8
            for (u32 i = 0; i < n; i++) acc = __fadd_rn(acc, (float)(threadIdx.x == 0 ? buf[i].x : buf[i].y));
        }
    }
    if (threadIdx.x < 2) mean[threadIdx.x] = __double2float_rn(__ddiv_rn((double)acc, (double)npx));
}

__global__ __launch_bounds__(256) void k_wb_apply(const uint8_t* __restrict__ src, size_t stride, u32 w, u32 npx, vp_tables tab,
                                                  const float* __restrict__ mean, uint8_t* __restrict__ dst)
{
    __shared__ WbLds s;
    load_wb_lds(s, tab);
    const float sa = __fsub_rn(mean[0], 128.0f), sb = __fsub_rn(mean[1], 128.0f);
    for (u32 p = blockIdx.x * 256 + threadIdx.x; p < npx; p += gridDim.x * 256) {
        const u32 y = p / w, x = p - y * w;
        wb_px(s, tab.abxz, src + (size_t)y * stride + 3 * (size_t)x, sa, sb, dst + 3 * (size_t)p);
    }
}

// ---- box mean ------------------------------------------------------------------------------------------------------------------------

// block = one row: inclusive prefix sums of a and b along the row (mod 2^32), 2048 pixels per step, 8 consecutive pixels per thread
__global__ __launch_bounds__(256) void k_wbb_row_prefix(const uint8_t* __restrict__ src, size_t stride, int w, vp_tables tab,
                                                        uint2* __restrict__ P)
{
    __shared__ LabLds s;
    __shared__ uint2 wtot[4];
    load_lab_lds(s, tab);
    __syncthreads();
    const int y = blockIdx.x;
    const uint8_t* row = src + (size_t)y * stride;
    uint2* prow = P + (size_t)y * w;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    u32 carry_a = 0, carry_b = 0;
    for (int x0 = 0; x0 < w; x0 += 2048) {
        const int xs = x0 + 8 * threadIdx.x;
        u32 pa[8], pb[8];
        u32 ta = 0, tb = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            int L, A = 0, B = 0;
            if (xs + k < w) lab_px<6>(s, row[3 * (xs + k)], row[3 * (xs + k) + 1], row[3 * (xs + k) + 2], L, A, B);
            ta += (u32)A; tb += (u32)B;
            pa[k] = ta; pb[k] = tb;
        }
        // exclusive scan of the thread totals: inside the wave, then across the four waves
        u32 ia = ta, ib = tb;
        for (int o = 1; o < 64; o <<= 1) {
            const u32 na = __shfl_up(ia, o), nb = __shfl_up(ib, o);
            if (lane >= o) { ia += na; ib += nb; }
        }
        if (lane == 63) wtot[wv] = make_uint2(ia, ib);
        __syncthreads();
        u32 oa = carry_a + ia - ta, ob = carry_b + ib - tb;
        for (int v = 0; v < wv; v++) { oa += wtot[v].x; ob += wtot[v].y; }
        carry_a += wtot[0].x + wtot[1].x + wtot[2].x + wtot[3].x;
        carry_b += wtot[0].y + wtot[1].y + wtot[2].y + wtot[3].y;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (xs + k < w) prow[xs + k] = make_uint2(oa + pa[k], ob + pb[k]);
    }
}

// the k-wide clamped window of row t around column x, from the row prefix sums
__device__ __forceinline__ uint2 row_box(const uint2* __restrict__ prow, int w, int x, int r)
{
    const int hi = x + r, lo = x - r - 1;
    uint2 v = prow[min(hi, w - 1)];
    if (lo >= 0) { const uint2 l = prow[lo]; v.x -= l.x; v.y -= l.y; }
    if (x - r < 0) {                       // r - x columns left of the image repeat column 0
        const uint2 a0 = prow[0];
        const u32 n = (u32)(r - x);
        v.x += n * a0.x; v.y += n * a0.y;
    }
    if (hi > w - 1) {                      // hi - (w - 1) columns right of it repeat column w - 1
        uint2 aw = prow[w - 1];
        if (w > 1) { const uint2 l = prow[w - 2]; aw.x -= l.x; aw.y -= l.y; }
        const u32 n = (u32)(hi - (w - 1));
        v.x += n * aw.x; v.y += n * aw.y;
    }
    return v;
}

// thread = (column x, tile of 64 rows): running column sums of the row windows inside the tile; the tile's total goes to T
__global__ __launch_bounds__(256) void k_wbb_col_prefix(const uint2* __restrict__ P, int w, int h, int r, uint2* __restrict__ Q,
                                                        uint2* __restrict__ T)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= w) return;
    const int t0 = blockIdx.y * WB_TILE, t1 = min(t0 + WB_TILE, h);
    uint2 acc = make_uint2(0, 0);
    for (int t = t0; t < t1; t++) {
        const uint2 v = row_box(P + (size_t)t * w, w, x, r);
        acc.x += v.x; acc.y += v.y;
        Q[(size_t)t * w + x] = acc;
    }
    T[(size_t)blockIdx.y * w + x] = acc;
}

// thread = column: the tile totals become exclusive carries, in place
__global__ __launch_bounds__(256) void k_wbb_carry(uint2* __restrict__ T, int w, int ntiles)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= w) return;
    uint2 acc = make_uint2(0, 0);
    for (int i = 0; i < ntiles; i++) {
        const uint2 v = T[(size_t)i * w + x];
        T[(size_t)i * w + x] = acc;
        acc.x += v.x; acc.y += v.y;
    }
}

// column prefix of the row windows down to row t (inclusive)
__device__ __forceinline__ uint2 col_prefix(const uint2* __restrict__ Q, const uint2* __restrict__ T, int w, int x, int t)
{
    const uint2 q = Q[(size_t)t * w + x], c = T[(size_t)(t / WB_TILE) * w + x];
    return make_uint2(q.x + c.x, q.y + c.y);
}

__global__ __launch_bounds__(256) void k_wbb_apply(const uint8_t* __restrict__ src, size_t stride, u32 w, int h, u32 npx, int r, double inv_area,
                                                   vp_tables tab, const uint2* __restrict__ Q, const uint2* __restrict__ T,
                                                   uint8_t* __restrict__ dst)
{
    __shared__ WbLds s;
    load_wb_lds(s, tab);
    for (u32 p = blockIdx.x * 256 + threadIdx.x; p < npx; p += gridDim.x * 256) {
        const int y = (int)(p / w), x = (int)(p - (u32)y * w);
        const int hi = y + r, lo = y - r - 1;
        uint2 v = col_prefix(Q, T, w, x, min(hi, h - 1));
        if (lo >= 0) { const uint2 l = col_prefix(Q, T, w, x, lo); v.x -= l.x; v.y -= l.y; }
        if (y - r < 0) {                   // rows above the image repeat row 0
            const uint2 a0 = Q[x];
            const u32 n = (u32)(r - y);
            v.x += n * a0.x; v.y += n * a0.y;
        }
        if (hi > h - 1) {                  // rows below it repeat row h - 1
            uint2 ah = col_prefix(Q, T, w, x, h - 1);
            if (h > 1) { const uint2 l = col_prefix(Q, T, w, x, h - 2); ah.x -= l.x; ah.y -= l.y; }
            const u32 n = (u32)(hi - (h - 1));
            v.x += n * ah.x; v.y += n * ah.y;
        }
        const float ma = __double2float_rn(__dmul_rn((double)v.x, inv_area)), mb = __double2float_rn(__dmul_rn((double)v.y, inv_area));
        wb_px(s, tab.abxz, src + (size_t)y * stride + 3 * (size_t)x, __fsub_rn(ma, 128.0f), __fsub_rn(mb, 128.0f), dst + 3 * (size_t)p);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------

static size_t wb_chunks(int w, int h) { return ((size_t)w * h + WB_CHUNK - 1) / WB_CHUNK; }
static size_t wb_tiles(int h) { return ((size_t)h + WB_TILE - 1) / WB_TILE; }

void vp_white_balance_want(vp_ws_frame& W, int w, int h, int kernel_size, vp_whitebal_ws* bw)
{
    const size_t npx = (size_t)w * h;
    if (kernel_size == VP_WB_GLOBAL_MEAN) { W.want(&bw->sums, wb_chunks(w, h) * sizeof(int2)); return; }
    W.want(&bw->P, npx * sizeof(uint2));
    W.want(&bw->Q, npx * sizeof(uint2));
    W.want(&bw->T, wb_tiles(h) * w * sizeof(uint2));
}

// d_mean: two floats of device memory (the global means; untouched by the box form)
int vpk_white_balance(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int kernel_size, uint8_t* d_dst, float* d_mean, const vp_whitebal_ws& bw)
{
    const size_t npx = (size_t)w * h;
    if (npx >= (1ull << 31)) return vp_fail(ctx, VP_ERR_UNSUPPORTED, "white balance: image above 2^31 pixels");
    const unsigned blocks = (unsigned)std::min<size_t>((npx + 255) / 256, (size_t)ctx->num_cu * 8);
    vp_prof_scope prof(ctx, VPK_COLOR);
    if (kernel_size == VP_WB_GLOBAL_MEAN) {
        const size_t nchunks = wb_chunks(w, h);
        int2* sums = bw.sums;
        hipLaunchKernelGGL(k_wb_chunk_sums, dim3((unsigned)nchunks), dim3(256), 0, ctx->stream, d_src, stride, (u32)w, (u32)npx, ctx->tab, sums);
        hipLaunchKernelGGL(k_wb_fold, dim3(1), dim3(64), 0, ctx->stream, (const int2*)sums, (u32)nchunks, (u32)npx, d_mean);
        hipLaunchKernelGGL(k_wb_apply, dim3(blocks), dim3(256), 0, ctx->stream, d_src, stride, (u32)w, (u32)npx, ctx->tab, (const float*)d_mean, d_dst);
    } else {
        const int r = kernel_size / 2;
        const size_t ntiles = wb_tiles(h);
        uint2 *P = bw.P, *Q = bw.Q, *T = bw.T;
        const double inv_area = 1.0 / (double)(kernel_size * kernel_size);
        const unsigned cols = (unsigned)((w + 255) / 256);
        hipLaunchKernelGGL(k_wbb_row_prefix, dim3((unsigned)h), dim3(256), 0, ctx->stream, d_src, stride, w, ctx->tab, P);
        hipLaunchKernelGGL(k_wbb_col_prefix, dim3(cols, (unsigned)ntiles), dim3(256), 0, ctx->stream, (const uint2*)P, w, h, r, Q, T);
        hipLaunchKernelGGL(k_wbb_carry, dim3(cols), dim3(256), 0, ctx->stream, T, w, (int)ntiles);
        hipLaunchKernelGGL(k_wbb_apply, dim3(blocks), dim3(256), 0, ctx->stream, d_src, stride, (u32)w, h, (u32)npx, r, inv_area, ctx->tab,
                           (const uint2*)Q, (const uint2*)T, d_dst);
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
