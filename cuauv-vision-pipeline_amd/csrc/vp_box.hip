// cv2.boxFilter / cv2.blur on uint8 images of 1..4 interleaved channels: dst[y][x][c] = cast(the sum of channel c of the
// border-extended source over the kh x kw window anchored at (kw / 2, kh / 2)); normalised, the byte OpenCV's roundings of sum / area
// agree on (vp_box_area_admit).  tests/box_pyr_restate.py is the statement.
//
// The image is rows of w * cn bytes whose horizontal neighbour is cn bytes away.  No loop is as long as the window:
//   row sums     a wave scans a staged row into per-channel prefix sums in LDS (uint16, modulo 2^16: a row sum is below 2^16): each
//                lane reads a chunk of bytes - a multiple of cn, so every lane starts at channel 0 -, sums it with stride cn, the
//                chunk totals are scanned across the wave with shuffles; a row sum is the difference of two prefix entries.
//   column sums  one thread per result column walks down the rows with a running sum: plus the row sum that enters, minus the one
//                that leaves.
// k_box (one pass): a block owns BX_TB result bytes x BX_TH rows and scans the BX_TH + kh - 1 rows of the tile and its halo once.
// k_box_rows + k_box_cols (two passes, where that halo does not fit the LDS: vp_box_make_plan): row sums of the whole image as uint16,
// then the column walk over strips of at least kh rows, so that the kh - 1 sums in front of a strip stay below the strip's own work.
#include "vp_box_dev.h"

static_assert(VP_BX_32S == VP_DEPTH_32S, "depth codes of vp.h");
static_assert(BX_CHUNK % 12 == 0 && BX_ROW_CHUNK % 12 == 0 && BX_TB == 256, "box: chunks are whole pixels of 1..4 channels, one thread per column");
static_assert(BX_MAXK * 255 < 65536, "box: a row sum fits uint16");

namespace {

// One wave scans bytes g0 .. g0 + 64 C of the extended row (lanes >= nchunks read nothing) into out[4 + i] = the sum of bytes
// i, i - CN, i - 2 CN, ... of that range modulo 2^16; out[0..3] = 0.  out is 4-byte aligned.
template <int CN, int C>
__device__ __forceinline__ void bx_scan_row(const uint8_t* row, int g0, int w, int border, int nchunks, uint16_t* out)
{
    const int lane = threadIdx.x & 63;
    u32 p[C];
    if (lane < nchunks) {
#pragma unroll
        for (int d = 0; d < C / 4; d++) {
            const u32 v = bx_ext4<CN>(row, g0 + lane * C + 4 * d, w, border);
#pragma unroll
            for (int k = 0; k < 4; k++) p[4 * d + k] = (v >> (8 * k)) & 255u;
        }
    } else {
#pragma unroll
        for (int i = 0; i < C; i++) p[i] = 0;
    }
#pragma unroll
    for (int i = CN; i < C; i++) p[i] += p[i - CN];
    u32 tot[CN], own[CN];
#pragma unroll
    for (int r = 0; r < CN; r++) tot[r] = own[r] = p[C - CN + r];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
        for (int r = 0; r < CN; r++) {
            const u32 t = __shfl_up(tot[r], off);
            if (lane >= off) tot[r] += t;
        }
    }
#pragma unroll
    for (int i = 0; i < C; i++) p[i] += tot[i % CN] - own[i % CN];
    u32* o32 = reinterpret_cast<u32*>(out);
    if (lane == 0) { o32[0] = 0; o32[1] = 0; }
    if (lane < nchunks) {
#pragma unroll
        for (int i = 0; i < C; i += 2) o32[2 + (lane * C + i) / 2] = (p[i] & 0xffffu) | (p[i + 1] << 16);
    }
}

struct bx_out {
    void* dst;
    int store;
    vp_box_div div;
    bool wide;                 // uint8: rows of whole dwords at 4-byte aligned addresses
};

// The result of column `col` (active: inside the row) of result row y; every lane of the wave calls it.
__device__ __forceinline__ void bx_emit(const bx_out& O, size_t rb, int y, int col, bool active, u32 sum)
{
    const size_t at = (size_t)y * rb + col;
    switch (O.store) {
        case VP_BX_STORE_8U:
        case VP_BX_STORE_8U_NORM: {
            const u32 v = O.store == VP_BX_STORE_8U ? min(sum, 255u) : vp_box_mean(sum, O.div);
            uint8_t* d = static_cast<uint8_t*>(O.dst);
            if (O.wide) {                                        // (rb % 4 == 0: the three columns after an active col % 4 == 0 are active)
                const u32 a = __shfl_down(v, 1), b = __shfl_down(v, 2), c = __shfl_down(v, 3);
                if (active && (col & 3) == 0) *reinterpret_cast<u32*>(d + at) = v | (a << 8) | (b << 16) | (c << 24);
            } else if (active) {
                d[at] = (uint8_t)v;
            }
            break;
        }
        case VP_BX_STORE_16S: if (active) static_cast<int16_t*>(O.dst)[at] = (int16_t)min(sum, 32767u); break;
        case VP_BX_STORE_32S: if (active) static_cast<int32_t*>(O.dst)[at] = (int32_t)sum; break;
        case VP_BX_STORE_32F: if (active) static_cast<float*>(O.dst)[at] = (float)sum; break;
        default: if (active) static_cast<double*>(O.dst)[at] = (double)sum; break;
    }
}

__device__ __forceinline__ bx_out bx_make_out(const vp_box_plan& P, void* dst, size_t rb)
{
    bx_out O;
    O.dst = dst; O.store = P.store; O.div = P.div;
    O.wide = ((((uintptr_t)dst) | rb) & 3u) == 0;
    return O;
}

// grid (P.gx, P.gy), 256 threads, P.lds_bytes of dynamic LDS
template <int CN>
__global__ __launch_bounds__(256) void k_box(const uint8_t* __restrict__ src, size_t sstride, int w, int h, vp_box_plan P, void* __restrict__ dst)
{
    extern __shared__ u32 bx_lds[];
    uint16_t* pre = reinterpret_cast<uint16_t*>(bx_lds);         // staged row j: pre[j * P.pitch ...], entry 4 + i is staged byte i
    const int rb = w * CN, b0 = blockIdx.x * BX_TB, y0 = blockIdx.y * BX_TH;
    const int nrows = min(BX_TH, h - y0), srows = nrows + P.kh - 1;
    for (int j = threadIdx.x >> 6; j < srows; j += 4) {
        const int yy = vp_deriv_border_index(y0 - P.ay + j, h, P.border);
        bx_scan_row<CN, BX_CHUNK>(yy < 0 ? nullptr : src + (size_t)yy * sstride, b0 - P.ax * CN, w, P.border, P.nchunks, pre + (size_t)j * P.pitch);
    }
    __syncthreads();
    const int t = threadIdx.x, col = b0 + t;
    const bool active = col < rb;
    const bx_out O = bx_make_out(P, dst, (size_t)rb);
    const uint16_t* hi = pre + 4 + t + (P.kw - 1) * CN;          // a row sum: the prefix at the window's last byte minus the one before its first
    const uint16_t* lo = pre + 4 + t - CN;
    u32 acc = 0;
    for (int j = 0; j < P.kh - 1; j++) acc += (u32)(uint16_t)(hi[j * P.pitch] - lo[j * P.pitch]);
    for (int r = 0; r < nrows; r++) {
        const int je = (r + P.kh - 1) * P.pitch, jl = r * P.pitch;
        acc += (u32)(uint16_t)(hi[je] - lo[je]);
        bx_emit(O, (size_t)rb, y0 + r, col, active, acc);
        acc -= (u32)(uint16_t)(hi[jl] - lo[jl]);
    }
}

// grid (P.gx, ceil(h / 4)), 256 threads: a wave = one image row, P.row_out row sums per block column.  mid: h x rb uint16.
template <int CN>
__global__ __launch_bounds__(256) void k_box_rows(const uint8_t* __restrict__ src, size_t sstride, int w, int h, vp_box_plan P, uint16_t* __restrict__ mid)
{
    constexpr int PITCH = 64 * BX_ROW_CHUNK + 4;
    __shared__ u32 lds[4 * PITCH / 2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint16_t* pre = reinterpret_cast<uint16_t*>(lds) + wave * PITCH;
    const int rb = w * CN, b0 = blockIdx.x * P.row_out, y = blockIdx.y * 4 + wave;
    bx_scan_row<CN, BX_ROW_CHUNK>(y < h ? src + (size_t)y * sstride : nullptr, b0 - P.ax * CN, w, P.border, 64, pre);
    __syncthreads();
    if (y >= h) return;
    const int n = min(P.row_out, rb - b0);
    uint16_t* m = mid + (size_t)y * rb + b0;
    for (int i = lane; i < n; i += 64) m[i] = (uint16_t)(pre[4 + i + (P.kw - 1) * CN] - pre[4 + i - CN]);
}

// grid (P.gx2, P.gy2), 256 threads: one thread per column, P.strip result rows per block
__global__ __launch_bounds__(256) void k_box_cols(const uint16_t* __restrict__ mid, int rb, int h, vp_box_plan P, void* __restrict__ dst)
{
    const int col = blockIdx.x * BX_TB + threadIdx.x, y0 = blockIdx.y * P.strip;
    const bool active = col < rb;
    const int nrows = min(P.strip, h - y0);
    const bx_out O = bx_make_out(P, dst, (size_t)rb);
    const uint16_t* m = mid + (active ? col : 0);
    auto rowsum = [&](int yy) -> u32 {
        const int yi = vp_deriv_border_index(yy, h, P.border);
        return yi < 0 ? 0u : (u32)m[(size_t)yi * rb];
    };
    u32 acc = 0;
    for (int j = 0; j < P.kh - 1; j++) acc += rowsum(y0 - P.ay + j);
    for (int r = 0; r < nrows; r++) {
        acc += rowsum(y0 - P.ay + r + P.kh - 1);
        bx_emit(O, (size_t)rb, y0 + r, col, active, acc);
        acc -= rowsum(y0 - P.ay + r);
    }
}

}  // namespace

size_t vp_box_mid_bytes(int w, int h, int cn, const vp_box_plan& P) { return P.onepass ? 0 : (size_t)w * cn * h * 2; }

// P: a plan vp_box_make_plan accepted for (w, h, cn), its div filled when it normalises; sstride: bytes between source rows; d_dst
// packed, P.esize bytes per element; d_mid: vp_box_mid_bytes of workspace (unused by the one-pass path)
int vpk_box_filter(vp_ctx* ctx, const uint8_t* d_src, size_t sstride, int w, int h, int cn, const vp_box_plan& P, uint16_t* d_mid, void* d_dst)
{
    vp_prof_scope ps(ctx, VPK_OTHER);
    hipStream_t s = ctx->stream;
    if (P.onepass) {
        const dim3 grid(P.gx, P.gy);
        switch (cn) {
            case 1: hipLaunchKernelGGL(k_box<1>, grid, dim3(256), P.lds_bytes, s, d_src, sstride, w, h, P, d_dst); break;
            case 2: hipLaunchKernelGGL(k_box<2>, grid, dim3(256), P.lds_bytes, s, d_src, sstride, w, h, P, d_dst); break;
            case 3: hipLaunchKernelGGL(k_box<3>, grid, dim3(256), P.lds_bytes, s, d_src, sstride, w, h, P, d_dst); break;
            default: hipLaunchKernelGGL(k_box<4>, grid, dim3(256), P.lds_bytes, s, d_src, sstride, w, h, P, d_dst); break;
        }
    } else {
        const dim3 grid(P.gx, P.gy);
        switch (cn) {
            case 1: hipLaunchKernelGGL(k_box_rows<1>, grid, dim3(256), 0, s, d_src, sstride, w, h, P, d_mid); break;
            case 2: hipLaunchKernelGGL(k_box_rows<2>, grid, dim3(256), 0, s, d_src, sstride, w, h, P, d_mid); break;
            case 3: hipLaunchKernelGGL(k_box_rows<3>, grid, dim3(256), 0, s, d_src, sstride, w, h, P, d_mid); break;
            default: hipLaunchKernelGGL(k_box_rows<4>, grid, dim3(256), 0, s, d_src, sstride, w, h, P, d_mid); break;
        }
        VP_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_box_cols, dim3(P.gx2, P.gy2), dim3(256), 0, s, d_mid, w * cn, h, P, d_dst);
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
