// cv2.integral of a uint8 image of 1..4 interleaved channels: dst is (h + 1) x (w + 1) x cn int32, row 0 and column 0 zero,
// dst[y + 1][x + 1][c] = the sum of channel c over rows 0..y and pixels 0..x.  tests/box_pyr_restate.py is the statement.
// Two passes over the result:
//   k_integral_rows  a wave = one result row: the zero row, or the zero pixel and the row's prefix sums.  Per step a wave scans
//                    IG_SCAN bytes: a lane sums its IG_CHUNK bytes (a multiple of cn) with stride cn, the chunk totals are scanned
//                    across the wave with shuffles, the last lane's totals are the carry into the next step.  The sums go through
//                    LDS so that the lanes store neighbouring int32.
//   k_integral_cols  one thread per result column adds the rows above, walking down, eight rows in flight.
#include "vp_box_dev.h"

namespace {

static_assert(IG_CHUNK % 12 == 0 && IG_SCAN == 64 * IG_CHUNK, "integral: chunks are whole pixels of 1..4 channels");

// grid ceil((h + 1) / 4), 256 threads
template <int CN>
__global__ __launch_bounds__(256) void k_integral_rows(const uint8_t* __restrict__ src, size_t sstride, int w, int h, int32_t* __restrict__ dst)
{
    __shared__ u32 buf[4][IG_SCAN];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int yo = blockIdx.x * 4 + wave, rb = w * CN;
    const bool live = yo <= h;
    int32_t* orow = dst + (size_t)(live ? yo : 0) * (size_t)(rb + CN);
    if (live && yo == 0)
        for (int i = lane; i < rb + CN; i += 64) orow[i] = 0;
    if (live && yo > 0 && lane < CN) orow[lane] = 0;
    const uint8_t* row = src + (size_t)(yo > 0 && live ? yo - 1 : 0) * sstride;
    const bool scan = live && yo > 0;
    u32 carry[CN];
#pragma unroll
    for (int r = 0; r < CN; r++) carry[r] = 0;
    for (int base = 0; base < rb; base += IG_SCAN) {             // (the same count in every wave: the barriers are uniform)
        u32 p[IG_CHUNK];
        const int g = base + lane * IG_CHUNK;
#pragma unroll
        for (int d = 0; d < IG_CHUNK / 4; d++) {
            u32 v = 0;
            if (scan) {
                if (g + 4 * d + 4 <= rb) v = bx_ld4(row + g + 4 * d);
                else
                    for (int k = 0; k < 4; k++)
                        if (g + 4 * d + k < rb) v |= (u32)row[g + 4 * d + k] << (8 * k);
            }
#pragma unroll
            for (int k = 0; k < 4; k++) p[4 * d + k] = (v >> (8 * k)) & 255u;
        }
#pragma unroll
        for (int i = CN; i < IG_CHUNK; i++) p[i] += p[i - CN];
        u32 tot[CN], own[CN];
#pragma unroll
        for (int r = 0; r < CN; r++) tot[r] = own[r] = p[IG_CHUNK - CN + r];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
            for (int r = 0; r < CN; r++) {
                const u32 t = __shfl_up(tot[r], off);
                if (lane >= off) tot[r] += t;
            }
        }
#pragma unroll
        for (int i = 0; i < IG_CHUNK; i++) buf[wave][lane * IG_CHUNK + i] = p[i] + tot[i % CN] - own[i % CN] + carry[i % CN];
#pragma unroll
        for (int r = 0; r < CN; r++) carry[r] += __shfl(tot[r], 63);
        __syncthreads();
        if (scan) {
            const int n = min(IG_SCAN, rb - base);
            for (int i = lane; i < n; i += 64) orow[CN + base + i] = (int32_t)buf[wave][i];
        }
        __syncthreads();
    }
}

// grid ceil((w + 1) * cn / IG_COLS), IG_COLS threads; ncol = (w + 1) * cn
__global__ __launch_bounds__(IG_COLS) void k_integral_cols(int32_t* __restrict__ dst, int ncol, int h)
{
    const int col = blockIdx.x * IG_COLS + threadIdx.x;
    if (col >= ncol) return;
    int32_t* p = dst + (size_t)ncol + col;                       // row 1
    int32_t acc = 0;
    int y = 0;
    for (; y + 8 <= h; y += 8) {
        int32_t v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = p[(size_t)(y + k) * ncol];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            acc += v[k];
            p[(size_t)(y + k) * ncol] = acc;
        }
    }
    for (; y < h; y++) {
        acc += p[(size_t)y * ncol];
        p[(size_t)y * ncol] = acc;
    }
}

}  // namespace

// d_dst: packed (h + 1) x (w + 1) x cn int32; vp_integral_sizes_ok(w, h, cn)
int vpk_integral(vp_ctx* ctx, const uint8_t* d_src, size_t sstride, int w, int h, int cn, int32_t* d_dst)
{
    vp_prof_scope ps(ctx, VPK_OTHER);
    const dim3 grid((unsigned)((h + 1 + 3) / 4));
    switch (cn) {
        case 1: hipLaunchKernelGGL(k_integral_rows<1>, grid, dim3(256), 0, ctx->stream, d_src, sstride, w, h, d_dst); break;
        case 2: hipLaunchKernelGGL(k_integral_rows<2>, grid, dim3(256), 0, ctx->stream, d_src, sstride, w, h, d_dst); break;
        case 3: hipLaunchKernelGGL(k_integral_rows<3>, grid, dim3(256), 0, ctx->stream, d_src, sstride, w, h, d_dst); break;
        default: hipLaunchKernelGGL(k_integral_rows<4>, grid, dim3(256), 0, ctx->stream, d_src, sstride, w, h, d_dst); break;
    }
    VP_HIP(ctx, hipGetLastError());
    const int ncol = (w + 1) * cn;
    hipLaunchKernelGGL(k_integral_cols, dim3((unsigned)((ncol + IG_COLS - 1) / IG_COLS)), dim3(IG_COLS), 0, ctx->stream, d_dst, ncol, h);
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
