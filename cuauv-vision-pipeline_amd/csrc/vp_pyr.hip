// cv2.pyrDown / cv2.pyrUp on uint8 images of 1..4 interleaved channels, one pass each; tests/box_pyr_restate.py is the statement.
//
// pyrDown: dst is ((w + 1) / 2, (h + 1) / 2); dst(y, x) = (sum_ij k_i k_j src(B(2y - 2 + i), B(2x - 2 + j)) + 128) >> 8, k = 1 4 6 4 1,
//   B = cv::borderInterpolate.  A block owns PD_TW x PD_TH result pixels: it stages the (2 PD_TH + 4) x (2 PD_TW + 4) source pixels
//   under them, border applied, runs the 5 taps along the rows at every second pixel into a uint16 plane (at most 16 * 255), then
//   down the columns at every second row.
// pyrUp: dst is (2w, 2h), in polyphase form: even results are s[x-1] + 6 s[x] + s[x+1], odd ones 4 (s[x] + s[x+1]), rows first
//   (uint16, at most 8 * 255), then columns with (.. + 32) >> 6.  Index -1 reads 1 (0 in a one-pixel image), index n reads n - 1
//   (vp_pyr_up_index).  A block owns PU_TW x PU_TH source pixels: stages (PU_TH + 2) x (PU_TW + 2), emits 2 PU_TH x 2 PU_TW.
// Both: a lane produces 4 neighbouring result bytes and stores them as one dword where the destination's rows are whole dwords at
// aligned addresses, byte by byte elsewhere and at a ragged tile end.
#include "vp_box_dev.h"

namespace {

static_assert((2 * PD_TW + 4) % 4 == 0 && PD_TW % 4 == 0 && PU_TW % 2 == 0, "pyr: staged rows and result rows in whole dwords");

__device__ __forceinline__ void pyr_store4(uint8_t* d, const u32* v, int n, bool wide)
{
    if (wide && n >= 4) {
        *reinterpret_cast<u32*>(d) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    } else {
        for (int e = 0; e < n && e < 4; e++) d[e] = (uint8_t)v[e];
    }
}

// grid (ceil(dw / PD_TW), ceil(dh / PD_TH)), 256 threads
template <int CN>
__global__ __launch_bounds__(256) void k_pyr_down(const uint8_t* __restrict__ src, size_t sstride, int w, int h, int border, uint8_t* __restrict__ dst)
{
    constexpr int SWB = (2 * PD_TW + 4) * CN, SROWS = 2 * PD_TH + 4, MW = PD_TW * CN;
    __shared__ u32 st32[SROWS * SWB / 4];
    __shared__ u32 mid32[SROWS * MW / 2];
    const uint8_t* st = reinterpret_cast<const uint8_t*>(st32);
    const int dw = (w + 1) / 2, dh = (h + 1) / 2;
    const int x0 = blockIdx.x * PD_TW, y0 = blockIdx.y * PD_TH;
    const int ncols = min(PD_TW, dw - x0), nrows = min(PD_TH, dh - y0);
    const int srows = 2 * nrows + 3, nb = ncols * CN;            // staged rows; result bytes per tile row
    const int ndw = ((2 * ncols + 3) * CN + 3) / 4;              // staged dwords per row <= SWB / 4
    for (int i = threadIdx.x; i < srows * ndw; i += 256) {
        const int j = i / ndw, d = i - j * ndw;
        const int yy = vp_deriv_border_index(2 * y0 - 2 + j, h, border);
        st32[j * (SWB / 4) + d] = bx_ext4<CN>(src + (size_t)yy * sstride, (2 * x0 - 2) * CN + 4 * d, w, border);
    }
    __syncthreads();
    const int nq = (nb + 3) / 4;                                 // lanes' groups of 4 result bytes per row
    for (int i = threadIdx.x; i < srows * nq; i += 256) {
        const int j = i / nq, o = 4 * (i - j * nq);
        u32 v[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int d = o + e, xl = d / CN, c = d - xl * CN;
            const uint8_t* p = st + j * SWB + 2 * xl * CN + c;
            v[e] = (u32)p[0] + p[4 * CN] + 4u * ((u32)p[CN] + p[3 * CN]) + 6u * p[2 * CN];
        }
        mid32[(j * MW + o) / 2] = v[0] | (v[1] << 16);
        mid32[(j * MW + o) / 2 + 1] = v[2] | (v[3] << 16);
    }
    __syncthreads();
    const size_t drb = (size_t)dw * CN;
    const bool wide = ((((uintptr_t)dst) | drb) & 3u) == 0;
    for (int i = threadIdx.x; i < nrows * nq; i += 256) {
        const int r = i / nq, o = 4 * (i - r * nq);
        u32 a[5][4];
#pragma unroll
        for (int t = 0; t < 5; t++) {
            const u32 lo = mid32[((2 * r + t) * MW + o) / 2], hi = mid32[((2 * r + t) * MW + o) / 2 + 1];
            a[t][0] = lo & 0xffffu; a[t][1] = lo >> 16; a[t][2] = hi & 0xffffu; a[t][3] = hi >> 16;
        }
        u32 v[4];
#pragma unroll
        for (int e = 0; e < 4; e++) v[e] = (a[0][e] + a[4][e] + 4u * (a[1][e] + a[3][e]) + 6u * a[2][e] + 128u) >> 8;
        pyr_store4(dst + (size_t)(y0 + r) * drb + (size_t)x0 * CN + o, v, nb - o, wide);
    }
}

// bytes g .. g + 3 of a source row under pyrUp's index map
template <int CN>
__device__ __forceinline__ u32 pu_ext4(const uint8_t* row, int g, int w)
{
    if (g >= 0 && g + 4 <= w * CN) return bx_ld4(row + g);
    u32 v = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int gb = g + k;
        const int px = (gb + 16 * CN) / CN - 16, c = gb - px * CN;           // (gb >= -CN)
        v |= (u32)row[(size_t)vp_pyr_up_index(px < -1 ? -1 : px, w) * CN + c] << (8 * k);
    }
    return v;
}

// grid (ceil(w / PU_TW), ceil(h / PU_TH)), 256 threads
template <int CN>
__global__ __launch_bounds__(256) void k_pyr_up(const uint8_t* __restrict__ src, size_t sstride, int w, int h, uint8_t* __restrict__ dst)
{
    constexpr int SWB = ((PU_TW + 2) * CN + 3) / 4 * 4, SROWS = PU_TH + 2, MW = 2 * PU_TW * CN;
    __shared__ u32 st32[SROWS * SWB / 4];
    __shared__ u32 mid32[SROWS * MW / 2];
    const uint8_t* st = reinterpret_cast<const uint8_t*>(st32);
    const int x0 = blockIdx.x * PU_TW, y0 = blockIdx.y * PU_TH;
    const int ncols = min(PU_TW, w - x0), nrows = min(PU_TH, h - y0);
    const int srows = nrows + 2, nb = 2 * ncols * CN;            // staged rows; result bytes per tile row
    const int ndw = ((ncols + 2) * CN + 3) / 4;
    for (int i = threadIdx.x; i < srows * ndw; i += 256) {
        const int j = i / ndw, d = i - j * ndw;
        const int yy = vp_pyr_up_index(y0 - 1 + j, h);
        st32[j * (SWB / 4) + d] = pu_ext4<CN>(src + (size_t)yy * sstride, (x0 - 1) * CN + 4 * d, w);
    }
    __syncthreads();
    const int nq = nb / 4 + ((nb & 3) ? 1 : 0);
    for (int i = threadIdx.x; i < srows * nq; i += 256) {
        const int j = i / nq, o = 4 * (i - j * nq);
        u32 v[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int d = o + e, dx = d / CN, c = d - dx * CN;
            const uint8_t* p = st + j * SWB + ((dx >> 1) + 1) * CN + c;      // the staged pixel under result pixel dx
            v[e] = (dx & 1) ? 4u * ((u32)p[0] + p[CN]) : (u32)p[-CN] + 6u * p[0] + p[CN];
        }
        mid32[(j * MW + o) / 2] = v[0] | (v[1] << 16);
        mid32[(j * MW + o) / 2 + 1] = v[2] | (v[3] << 16);
    }
    __syncthreads();
    const size_t drb = (size_t)2 * w * CN;
    const bool wide = ((((uintptr_t)dst) | drb) & 3u) == 0;
    for (int i = threadIdx.x; i < 2 * nrows * nq; i += 256) {
        const int dr = i / nq, o = 4 * (i - dr * nq), r = dr >> 1;
        u32 a[3][4];
#pragma unroll
        for (int t = 0; t < 3; t++) {
            const u32 lo = mid32[((r + t) * MW + o) / 2], hi = mid32[((r + t) * MW + o) / 2 + 1];
            a[t][0] = lo & 0xffffu; a[t][1] = lo >> 16; a[t][2] = hi & 0xffffu; a[t][3] = hi >> 16;
        }
        u32 v[4];
#pragma unroll
        for (int e = 0; e < 4; e++) v[e] = ((dr & 1) ? 4u * (a[1][e] + a[2][e]) + 32u : a[0][e] + 6u * a[1][e] + a[2][e] + 32u) >> 6;
        pyr_store4(dst + (size_t)(2 * y0 + dr) * drb + (size_t)2 * x0 * CN + o, v, nb - o, wide);
    }
}

}  // namespace

// d_dst: packed ((w + 1) / 2) x ((h + 1) / 2) x cn; border: REFLECT_101, REPLICATE or REFLECT
int vpk_pyr_down(vp_ctx* ctx, const uint8_t* d_src, size_t sstride, int w, int h, int cn, int border, uint8_t* d_dst)
{
    vp_prof_scope ps(ctx, VPK_OTHER);
    const dim3 grid((unsigned)(((w + 1) / 2 + PD_TW - 1) / PD_TW), (unsigned)(((h + 1) / 2 + PD_TH - 1) / PD_TH));
    switch (cn) {
        case 1: hipLaunchKernelGGL(k_pyr_down<1>, grid, dim3(256), 0, ctx->stream, d_src, sstride, w, h, border, d_dst); break;
        case 2: hipLaunchKernelGGL(k_pyr_down<2>, grid, dim3(256), 0, ctx->stream, d_src, sstride, w, h, border, d_dst); break;
        case 3: hipLaunchKernelGGL(k_pyr_down<3>, grid, dim3(256), 0, ctx->stream, d_src, sstride, w, h, border, d_dst); break;
        default: hipLaunchKernelGGL(k_pyr_down<4>, grid, dim3(256), 0, ctx->stream, d_src, sstride, w, h, border, d_dst); break;
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

// d_dst: packed 2w x 2h x cn
int vpk_pyr_up(vp_ctx* ctx, const uint8_t* d_src, size_t sstride, int w, int h, int cn, uint8_t* d_dst)
{
    vp_prof_scope ps(ctx, VPK_OTHER);
    const dim3 grid((unsigned)((w + PU_TW - 1) / PU_TW), (unsigned)((h + PU_TH - 1) / PU_TH));
    switch (cn) {
        case 1: hipLaunchKernelGGL(k_pyr_up<1>, grid, dim3(256), 0, ctx->stream, d_src, sstride, w, h, d_dst); break;
        case 2: hipLaunchKernelGGL(k_pyr_up<2>, grid, dim3(256), 0, ctx->stream, d_src, sstride, w, h, d_dst); break;
        case 3: hipLaunchKernelGGL(k_pyr_up<3>, grid, dim3(256), 0, ctx->stream, d_src, sstride, w, h, d_dst); break;
        default: hipLaunchKernelGGL(k_pyr_up<4>, grid, dim3(256), 0, ctx->stream, d_src, sstride, w, h, d_dst); break;
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
