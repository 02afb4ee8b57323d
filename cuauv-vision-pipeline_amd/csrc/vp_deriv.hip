// cv2.Sobel / Scharr / Laplacian / spatialGradient on uint8 images, scale = 1, delta = 0: dst[y][x][c] = saturate_cast<T>(the integer
// correlation of channel c of the border-extended source with the operator's unnormalised integer kernel).  Every OpenCV path of
// these filters produces that integer before its final cast (the sums stay below 2^24 where it keeps them in floats), so the result
// equals OpenCV's by construction; tests/deriv_restate.py is the statement.
//
// The image is rows of w * cn bytes whose horizontal neighbour is cn bytes away; channels never mix.  The source has a row stride, the
// destination is packed.  One pass: a block of 256 threads owns a tile of DV_TB result bytes x DV_TH rows and
//   1. stages the tile and its halo of K / 2 pixels in LDS, the border already applied (vp_deriv_border_index), from 4-byte reads at
//      aligned addresses whatever the source pointer and stride are (the staging of k_median_net);
//   2. runs the row filter over every staged row into an int16 plane in LDS (a row sum is at most 64 * 255 = 16,320 in magnitude),
//      8 neighbouring results per thread and one 16-byte LDS store;
//   3. runs the column filter out of that plane in int32 (at most 64 * 64 * 255 < 2^21), 8 neighbouring results per lane from one
//      16-byte LDS load per tap, casts and stores them as 8 bytes (uint8) or as 16-byte stores (one for int16, two for float, four for
//      double); a row of the destination that is not aligned for that, and a ragged tile end, are stored element by element.
// k_deriv<K, MODE, T>: K taps (values are kernel arguments, the counts and T compile-time); MODE ONE = one separable term (Sobel,
// Scharr), SUM = two terms added (Laplacian 5 and 7: Sobel(2,0) + Sobel(0,2)), PAIR = two terms to two planes (spatialGradient).
// k_lap3<T>: the 3x3 Laplacians (ksize 1 and 3) straight from the staged bytes, no row plane.
#include "vp_internal.h"
#include "vp_deriv_plan.h"

static_assert(VP_DV_OP_SOBEL == VP_DERIV_SOBEL && VP_DV_OP_SCHARR == VP_DERIV_SCHARR && VP_DV_OP_LAPLACIAN == VP_DERIV_LAPLACIAN, "operator codes of vp.h");
static_assert(VP_DV_8U == VP_DEPTH_8U && VP_DV_16S == VP_DEPTH_16S && VP_DV_32F == VP_DEPTH_32F && VP_DV_64F == VP_DEPTH_64F, "depth codes of vp.h");
static_assert(VP_DV_CONSTANT == VP_BORDER_CONSTANT && VP_DV_REPLICATE == VP_BORDER_REPLICATE && VP_DV_REFLECT == VP_BORDER_REFLECT &&
              VP_DV_REFLECT_101 == VP_BORDER_REFLECT_101 && VP_DV_ISOLATED == VP_BORDER_ISOLATED, "border codes of vp.h");

namespace {

#define DV_SW (DV_TB + 2 * DV_PAD + 4)             // staged bytes per row: tile, halo, and up to 3 bytes that bring the row's dwords to aligned addresses
#define DV_SH(K) (DV_TH + (K) - 1)                 // staged rows
static_assert(DV_PAD >= (DV_MAXK / 2) * 4 && DV_PAD % 4 == 0 && DV_SW % 4 == 0, "k_deriv: the halo of four channels in whole dwords");
static_assert(DV_TB == 64 * DV_EPL && DV_EPL == 8 && DV_TH % 4 == 0, "k_deriv: one wave per result row, 8 results per lane");
static_assert(DV_SH(DV_MAXK) * DV_SW + 2 * DV_SH(DV_MAXK) * DV_TB * 2 <= 64 * 1024, "k_deriv: static LDS above 64 KiB");
static_assert(64 * 255 <= 32767, "k_deriv: a row sum of the largest smoothing kernel fits the int16 plane");

enum { DV_ONE = VP_DV_KERNEL_ONE, DV_SUM = VP_DV_KERNEL_SUM, DV_PAIR = VP_DV_KERNEL_PAIR };

struct dv_tile {
    const uint8_t* src;
    size_t sstride;
    int w, h, cn, border;
    int rb, b0, y0, nb, nrows;     // row bytes; the tile's first result byte and row; its result bytes and rows
    uintptr_t base;
};

// the image row that staged row j of a halo of R reads (-1: the constant border), and the 0..3 bytes its staging is shifted by
template <int R>
__device__ __forceinline__ int dv_src_row(const dv_tile& T, int j) { return vp_deriv_border_index(T.y0 - R + j, T.h, T.border); }
__device__ __forceinline__ int dv_shift(const dv_tile& T, int yy) { return yy < 0 ? 0 : (int)((T.base + (size_t)yy * T.sstride) & 3u); }

__device__ __forceinline__ dv_tile dv_make_tile(const uint8_t* src, size_t sstride, int w, int h, int cn, int border)
{
    dv_tile T;
    T.src = src; T.sstride = sstride; T.w = w; T.h = h; T.cn = cn; T.border = border;
    T.rb = w * cn;
    T.b0 = blockIdx.x * DV_TB;
    T.y0 = blockIdx.y * DV_TH;
    T.nb = min(DV_TB, T.rb - T.b0);
    T.nrows = min(DV_TH, h - T.y0);
    T.base = (uintptr_t)src + (uintptr_t)(intptr_t)(T.b0 - DV_PAD);
    return T;
}

// Staged byte s of staged row j is byte b0 - DV_PAD - shift + s of the extended image row; a constant-border row or byte is 0.
template <int R>
__device__ __forceinline__ void dv_stage(const dv_tile& T, u32* st32)
{
    const int sh = T.nrows + 2 * R;                          // staged rows <= DV_SH(2 R + 1)
    const int ndw = (T.nb + 2 * DV_PAD + 3 + 3) / 4;         // staged dwords per row <= DV_SW / 4
    for (int i = threadIdx.x; i < sh * ndw; i += 256) {
        const int j = i / ndw, d = i - j * ndw;
        const int yy = dv_src_row<R>(T, j);
        u32 v = 0;
        if (yy >= 0) {
            const uint8_t* row = T.src + (size_t)yy * T.sstride;
            const int g = T.b0 - DV_PAD - dv_shift(T, yy) + 4 * d;
            if (g >= 0 && g + 4 <= T.rb) {
                v = *reinterpret_cast<const u32*>(row + g);
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) {                // a byte left or right of the row is its channel of the pixel the border maps to
                    const int gb = g + k;
                    const int px = (gb + 16 * T.cn) / T.cn - 16, c = gb - px * T.cn;      // (gb >= -DV_PAD - 3)
                    const int pm = vp_deriv_border_index(px, T.w, T.border);
                    if (pm >= 0) v |= (u32)row[(size_t)pm * T.cn + c] << (8 * k);
                }
            }
        }
        st32[j * (DV_SW / 4) + d] = v;
    }
}

__device__ __forceinline__ u32 dv_pack16(int lo, int hi) { return ((u32)lo & 0xffffu) | ((u32)hi << 16); }
__device__ __forceinline__ int dv_lo16(u32 v) { return (int)(short)(v & 0xffffu); }
__device__ __forceinline__ int dv_hi16(u32 v) { return (int)v >> 16; }

template <typename T> __device__ __forceinline__ T dv_cast(int v);
template <> __device__ __forceinline__ uint8_t dv_cast<uint8_t>(int v) { return (uint8_t)min(max(v, 0), 255); }
template <> __device__ __forceinline__ int16_t dv_cast<int16_t>(int v) { return (int16_t)min(max(v, -32768), 32767); }
template <> __device__ __forceinline__ float dv_cast<float>(int v) { return (float)v; }
template <> __device__ __forceinline__ double dv_cast<double>(int v) { return (double)v; }

// whether the 8 results of a lane can leave as vector stores: every destination row starts at a multiple of the store's width
template <typename T>
__device__ __forceinline__ bool dv_rows_aligned(const T* dst, int rb)
{
    constexpr unsigned A = sizeof(T) == 1 ? 8u : 16u;
    return ((((uintptr_t)dst) | ((uintptr_t)rb * sizeof(T))) & (A - 1u)) == 0;
}

// the n <= 8 results of one lane; wide: n == 8 and d is aligned as dv_rows_aligned says
template <typename T>
__device__ __forceinline__ void dv_store(T* d, const int* acc, int n, bool wide)
{
    if (!wide) {
        for (int e = 0; e < n; e++) d[e] = dv_cast<T>(acc[e]);
        return;
    }
    if constexpr (sizeof(T) == 1) {
        u32 lo = 0, hi = 0;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            lo |= (u32)dv_cast<T>(acc[e]) << (8 * e);
            hi |= (u32)dv_cast<T>(acc[4 + e]) << (8 * e);
        }
        *reinterpret_cast<uint2*>(d) = make_uint2(lo, hi);
    } else if constexpr (sizeof(T) == 2) {
        vp_store16(d, dv_pack16(dv_cast<T>(acc[0]), dv_cast<T>(acc[1])), dv_pack16(dv_cast<T>(acc[2]), dv_cast<T>(acc[3])),
                   dv_pack16(dv_cast<T>(acc[4]), dv_cast<T>(acc[5])), dv_pack16(dv_cast<T>(acc[6]), dv_cast<T>(acc[7])));
    } else if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int e = 0; e < 8; e += 4)
            vp_store16(d + e, __float_as_uint((float)acc[e]), __float_as_uint((float)acc[e + 1]), __float_as_uint((float)acc[e + 2]), __float_as_uint((float)acc[e + 3]));
    } else {
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
            const u64 a = (u64)__double_as_longlong((double)acc[e]), b = (u64)__double_as_longlong((double)acc[e + 1]);
            vp_store16(d + e, (u32)a, (u32)(a >> 32), (u32)b, (u32)(b >> 32));
        }
    }
}

// grid (ceil(w * cn / DV_TB), ceil(h / DV_TH)), 256 threads.  dst2: the second plane of MODE PAIR.
template <int K, int MODE, typename T>
__global__ __launch_bounds__(256) void k_deriv(const uint8_t* __restrict__ src, size_t sstride, int w, int h, int cn, int border, vp_deriv_taps taps,
                                               T* __restrict__ dst, T* __restrict__ dst2)
{
    constexpr int R = K / 2, NPL = MODE == DV_ONE ? 1 : 2, PLANE = DV_SH(K) * DV_TB;
    __shared__ u32 st32[DV_SH(K) * (DV_SW / 4)];
    __shared__ uint4 mid4[NPL * PLANE / 8];
    const uint8_t* st = reinterpret_cast<const uint8_t*>(st32);
    const dv_tile tile = dv_make_tile(src, sstride, w, h, cn, border);
    dv_stage<R>(tile, st32);
    __syncthreads();
    const int sh = tile.nrows + 2 * R;
    // row filter: staged row j, results o .. o + 7 of the tile
    for (int i = threadIdx.x; i < sh * 64; i += 256) {
        const int j = i >> 6, o = DV_EPL * (i & 63);
        if (o >= tile.nb) continue;
        const uint8_t* p = st + j * DV_SW + DV_PAD + dv_shift(tile, dv_src_row<R>(tile, j)) + o - R * cn;
        int a[DV_EPL], b[DV_EPL];
#pragma unroll
        for (int e = 0; e < DV_EPL; e++) a[e] = b[e] = 0;
#pragma unroll
        for (int t = 0; t < K; t++) {
#pragma unroll
            for (int e = 0; e < DV_EPL; e++) {
                const int v = p[e + t * cn];
                a[e] += taps.rowA[t] * v;
                if constexpr (NPL == 2) b[e] += taps.rowB[t] * v;
            }
        }
        mid4[(j * DV_TB + o) / 8] = make_uint4(dv_pack16(a[0], a[1]), dv_pack16(a[2], a[3]), dv_pack16(a[4], a[5]), dv_pack16(a[6], a[7]));
        if constexpr (NPL == 2)
            mid4[(PLANE + j * DV_TB + o) / 8] = make_uint4(dv_pack16(b[0], b[1]), dv_pack16(b[2], b[3]), dv_pack16(b[4], b[5]), dv_pack16(b[6], b[7]));
    }
    __syncthreads();
    // column filter: a wave = one result row, lane q has its results o .. o + 7
    const int o = DV_EPL * (threadIdx.x & 63);
    if (o >= tile.nb) return;
    const int n = min(DV_EPL, tile.nb - o);
    const bool wide = n == DV_EPL && dv_rows_aligned(dst, tile.rb) && (MODE != DV_PAIR || dv_rows_aligned(dst2, tile.rb));
    for (int r = threadIdx.x >> 6; r < tile.nrows; r += 4) {
        int acc[DV_EPL], acc2[DV_EPL];
#pragma unroll
        for (int e = 0; e < DV_EPL; e++) acc[e] = acc2[e] = 0;
#pragma unroll
        for (int t = 0; t < K; t++) {
            const uint4 va = mid4[((r + t) * DV_TB + o) / 8];
            const u32 wa[4] = {va.x, va.y, va.z, va.w};
#pragma unroll
            for (int e = 0; e < 4; e++) {
                acc[2 * e] += taps.colA[t] * dv_lo16(wa[e]);
                acc[2 * e + 1] += taps.colA[t] * dv_hi16(wa[e]);
            }
            if constexpr (NPL == 2) {
                const uint4 vb = mid4[(PLANE + (r + t) * DV_TB + o) / 8];
                const u32 wb[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    if constexpr (MODE == DV_SUM) {
                        acc[2 * e] += taps.colB[t] * dv_lo16(wb[e]);
                        acc[2 * e + 1] += taps.colB[t] * dv_hi16(wb[e]);
                    } else {
                        acc2[2 * e] += taps.colB[t] * dv_lo16(wb[e]);
                        acc2[2 * e + 1] += taps.colB[t] * dv_hi16(wb[e]);
                    }
                }
            }
        }
        const size_t at = (size_t)(tile.y0 + r) * tile.rb + tile.b0 + o;
        dv_store<T>(dst + at, acc, n, wide);
        if constexpr (MODE == DV_PAIR) dv_store<T>(dst2 + at, acc2, n, wide);
    }
}

// the 3x3 Laplacians: corner, edge and centre weights (ksize 1: 0, 1, -4; ksize 3: 2, 0, -8).  Same grid.
template <typename T>
__global__ __launch_bounds__(256) void k_lap3(const uint8_t* __restrict__ src, size_t sstride, int w, int h, int cn, int border, int wc, int we, int wm,
                                              T* __restrict__ dst)
{
    __shared__ u32 st32[DV_SH(3) * (DV_SW / 4)];
    const uint8_t* st = reinterpret_cast<const uint8_t*>(st32);
    const dv_tile tile = dv_make_tile(src, sstride, w, h, cn, border);
    dv_stage<1>(tile, st32);
    __syncthreads();
    const int o = DV_EPL * (threadIdx.x & 63);
    if (o >= tile.nb) return;
    const int n = min(DV_EPL, tile.nb - o);
    const bool wide = n == DV_EPL && dv_rows_aligned(dst, tile.rb);
    for (int r = threadIdx.x >> 6; r < tile.nrows; r += 4) {
        const uint8_t* p[3];                                 // per window row: the tap left of result o
#pragma unroll
        for (int dy = 0; dy < 3; dy++) p[dy] = st + (r + dy) * DV_SW + DV_PAD + dv_shift(tile, dv_src_row<1>(tile, r + dy)) + o - cn;
        int acc[DV_EPL];
#pragma unroll
        for (int e = 0; e < DV_EPL; e++) {
            const int corners = p[0][e] + p[0][e + 2 * cn] + p[2][e] + p[2][e + 2 * cn];
            const int edges = p[0][e + cn] + p[1][e] + p[1][e + 2 * cn] + p[2][e + cn];
            acc[e] = wc * corners + we * edges + wm * p[1][e + cn];
        }
        dv_store<T>(dst + (size_t)(tile.y0 + r) * tile.rb + tile.b0 + o, acc, n, wide);
    }
}

template <int MODE, typename T>
void dv_launch_k(int K, dim3 grid, hipStream_t s, const uint8_t* src, size_t sstride, int w, int h, int cn, int border, const vp_deriv_taps& taps, T* dst, T* dst2)
{
    if (K == 3) hipLaunchKernelGGL((k_deriv<3, MODE, T>), grid, dim3(256), 0, s, src, sstride, w, h, cn, border, taps, dst, dst2);
    else if (K == 5) hipLaunchKernelGGL((k_deriv<5, MODE, T>), grid, dim3(256), 0, s, src, sstride, w, h, cn, border, taps, dst, dst2);
    else hipLaunchKernelGGL((k_deriv<7, MODE, T>), grid, dim3(256), 0, s, src, sstride, w, h, cn, border, taps, dst, dst2);
}

template <typename T>
void dv_launch(vp_ctx* ctx, const vp_deriv_plan& P, const uint8_t* src, size_t sstride, int w, int h, int cn, void* dst)
{
    const dim3 grid(P.gx, P.gy);
    T* d = static_cast<T*>(dst);
    if (P.kernel == VP_DV_KERNEL_LAP3)
        hipLaunchKernelGGL(k_lap3<T>, grid, dim3(256), 0, ctx->stream, src, sstride, w, h, cn, P.border, P.lap_corner, P.lap_edge, P.lap_centre, d);
    else if (P.kernel == VP_DV_KERNEL_SUM)
        dv_launch_k<DV_SUM, T>(P.K, grid, ctx->stream, src, sstride, w, h, cn, P.border, P.taps, d, nullptr);
    else
        dv_launch_k<DV_ONE, T>(P.K, grid, ctx->stream, src, sstride, w, h, cn, P.border, P.taps, d, nullptr);
}

}  // namespace

// P: a plan vp_deriv_make_plan accepted for (w, h, cn); sstride: bytes between source rows; d_dst: packed, P.esize bytes per element;
// d_dst2: the dy plane of VP_DV_KERNEL_PAIR (d_dst is dx), else unused
int vpk_deriv(vp_ctx* ctx, const uint8_t* d_src, size_t sstride, int w, int h, int cn, const vp_deriv_plan& P, void* d_dst, void* d_dst2)
{
    vp_prof_scope ps(ctx, VPK_OTHER);
    if (P.kernel == VP_DV_KERNEL_PAIR) {
        hipLaunchKernelGGL((k_deriv<3, DV_PAIR, int16_t>), dim3(P.gx, P.gy), dim3(256), 0, ctx->stream, d_src, sstride, w, h, cn, P.border, P.taps,
                           static_cast<int16_t*>(d_dst), static_cast<int16_t*>(d_dst2));
    } else {
        switch (P.depth) {
            case VP_DV_8U: dv_launch<uint8_t>(ctx, P, d_src, sstride, w, h, cn, d_dst); break;
            case VP_DV_16S: dv_launch<int16_t>(ctx, P, d_src, sstride, w, h, cn, d_dst); break;
            case VP_DV_32F: dv_launch<float>(ctx, P, d_src, sstride, w, h, cn, d_dst); break;
            default: dv_launch<double>(ctx, P, d_src, sstride, w, h, cn, d_dst); break;
        }
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
