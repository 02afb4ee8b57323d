// cv2.remap, cv2.convertMaps and cv2.warpPerspective on 8-bit images of 1..4 channels, OpenCV's classical fixed-point path (every
// release up to 4.10; DESIGN.md section 4.21 has the arithmetic statement by statement).
//
// Every source coordinate becomes an int16 integer part and a 5 + 5 bit fraction index (fy * 32 + fx); a linear sample blends the
// four neighbours with the 15-bit weights (32 - fx)(32 - fy) 32, ... and rounds (sum + 2^14) >> 15, exactly what k_warp_affine_u8
// (vp_yolo.hip) does after its own coordinate arithmetic; a nearest sample reads one pixel.  BORDER_CONSTANT substitutes the border
// value per neighbour, BORDER_REPLICATE clamps the neighbour's coordinates.  What differs between the kernels is where the coordinates
// come from: the fixed form in HBM (k_remap_fixed), float maps converted in registers (k_remap_f32, the same bytes as k_convert_maps
// followed by k_remap_fixed), or a 3x3 matrix evaluated in double per pixel (k_warp_perspective).
//
// Float map values must be finite with |v| * 32 < 2^31.  Outside that cv2 gives what x86's cvtss2si gives (INT_MIN, the "integer
// indefinite"); rm_round_f returns the same, but nothing is promised there.
//
// The kernels are memory-bound gathers: one lane owns RM_PPT adjacent destination pixels, so its map loads are 16 bytes (8 of
// fractions) and its store is 4 * cn bytes wherever rows are whole groups of RM_PPT pixels and the pointers are 16-byte aligned
// (`vec`); ragged rows and unaligned pointers take scalar loads and byte stores.  No LDS: the maps of real lenses are smooth and the
// taps of neighbouring lanes share cache lines.
#include "vp_internal.h"
#include "vp_remap_plan.h"

#include <climits>
#include <cmath>

struct rm_src { const uint8_t* p; size_t stride; int w, h, border; uint8_t cval[4]; };

__device__ __forceinline__ int rm_sat16(int v) { return min(max(v, -32768), 32767); }
// cvRound(float): round half to even; out of range and NaN as x86
__device__ __forceinline__ int rm_round_f(float v)
{
    if (!(v >= -2147483648.f && v < 2147483648.f)) return INT_MIN;
    return (int)rintf(v);
}
// a float map entry -> integer parts and fraction index (cv::remap's per-block conversion = cv::convertMaps)
template <bool LINEAR>
__device__ __forceinline__ void rm_convert(float mx, float my, int& sx, int& sy, int& frac)
{
    if (LINEAR) {
        const int ix = rm_round_f(__fmul_rn(mx, 32.f)), iy = rm_round_f(__fmul_rn(my, 32.f));
        sx = rm_sat16(ix >> 5); sy = rm_sat16(iy >> 5);
        frac = (iy & 31) * 32 + (ix & 31);
    } else {
        sx = rm_sat16(rm_round_f(mx)); sy = rm_sat16(rm_round_f(my));
        frac = 0;
    }
}

// The one sampling function of the gather kernels: the pixel at (sx, sy) + fraction index `frac` of source S -> o[0..CN).
// Every address that is dereferenced lies inside the source: a coordinate is clamped (replicate) or tested (constant) first.
template <int CN, bool LINEAR>
__device__ __forceinline__ void rm_sample(const rm_src& S, int sx, int sy, int frac, uint8_t* o)
{
    const int sw = S.w, sh = S.h;
    if (!LINEAR) {
        bool in = (unsigned)sx < (unsigned)sw && (unsigned)sy < (unsigned)sh;
        if (S.border == VP_BORDER_REPLICATE) {
            sx = min(max(sx, 0), sw - 1); sy = min(max(sy, 0), sh - 1);
            in = true;
        }
        if (in) {
            const uint8_t* p = S.p + (size_t)sy * S.stride + (size_t)sx * CN;
#pragma unroll
            for (int c = 0; c < CN; c++) o[c] = p[c];
        } else {
#pragma unroll
            for (int c = 0; c < CN; c++) o[c] = S.cval[c];
        }
        return;
    }
    const int fx = frac & 31, fy = (frac >> 5) & 31;
    const int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32, w10 = (32 - fx) * fy * 32, w11 = fx * fy * 32;
    if (S.border == VP_BORDER_CONSTANT && (sx >= sw || sx + 1 < 0 || sy >= sh || sy + 1 < 0)) {
#pragma unroll
        for (int c = 0; c < CN; c++) o[c] = S.cval[c];
        return;
    }
    int x0, x1, y0, y1;
    if (S.border == VP_BORDER_REPLICATE) {
        x0 = min(max(sx, 0), sw - 1); x1 = min(max(sx + 1, 0), sw - 1);
        y0 = min(max(sy, 0), sh - 1); y1 = min(max(sy + 1, 0), sh - 1);
    } else {
        x0 = (sx >= 0 && sx < sw) ? sx : -1; x1 = (sx + 1 >= 0 && sx + 1 < sw) ? sx + 1 : -1;
        y0 = (sy >= 0 && sy < sh) ? sy : -1; y1 = (sy + 1 >= 0 && sy + 1 < sh) ? sy + 1 : -1;
    }
    const bool i00 = x0 >= 0 && y0 >= 0, i01 = x1 >= 0 && y0 >= 0, i10 = x0 >= 0 && y1 >= 0, i11 = x1 >= 0 && y1 >= 0;
    const uint8_t* r0 = S.p + (size_t)max(y0, 0) * S.stride;
    const uint8_t* r1 = S.p + (size_t)max(y1, 0) * S.stride;
    const size_t c0 = (size_t)max(x0, 0) * CN, c1 = (size_t)max(x1, 0) * CN;
#pragma unroll
    for (int c = 0; c < CN; c++) {
        const int cv = S.cval[c];
        const int v00 = i00 ? r0[c0 + c] : cv, v01 = i01 ? r0[c1 + c] : cv, v10 = i10 ? r1[c0 + c] : cv, v11 = i11 ? r1[c1 + c] : cv;
        const int v = (v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11 + (1 << 14)) >> 15;
        o[c] = (uint8_t)min(max(v, 0), 255);
    }
}

// n <= RM_PPT pixels of CN bytes to d.  vec: n == RM_PPT and d is aligned to its store (4 bytes for CN 1 and 3, 8 for 2, 16 for 4)
template <int CN>
__device__ __forceinline__ void rm_store(uint8_t* d, const uint8_t* o, bool vec, int n)
{
    if (vec) {
        u32 q[CN];
#pragma unroll
        for (int i = 0; i < CN; i++) q[i] = (u32)o[4 * i] | ((u32)o[4 * i + 1] << 8) | ((u32)o[4 * i + 2] << 16) | ((u32)o[4 * i + 3] << 24);
        if constexpr (CN == 1) *(u32*)d = q[0];
        else if constexpr (CN == 2) *(uint2*)d = make_uint2(q[0], q[1]);
        else if constexpr (CN == 3) { u32* p = (u32*)d; p[0] = q[0]; p[1] = q[1]; p[2] = q[2]; }
        else *(uint4*)d = make_uint4(q[0], q[1], q[2], q[3]);
        return;
    }
#pragma unroll
    for (int i = 0; i < RM_PPT; i++)
        if (i < n) {
#pragma unroll
            for (int c = 0; c < CN; c++) d[i * CN + c] = o[i * CN + c];
        }
}

// the lane's first destination pixel; false: nothing to do
__device__ __forceinline__ bool rm_lane(int dw, int dh, int& x0, int& y, int& n)
{
    x0 = (int)(blockIdx.x * 64 + threadIdx.x) * RM_PPT;
    y = (int)(blockIdx.y * RM_TH + threadIdx.y);
    if (x0 >= dw || y >= dh) return false;
    n = min(RM_PPT, dw - x0);
    return true;
}

// dst(y, x) = sample of S at xy(y, x) [+ fraction index frac(y, x) & 1023].  grid (ceil(mw / RM_TW), ceil(mh / RM_TH)), block (64, RM_TH).
template <int CN, bool LINEAR>
__global__ __launch_bounds__(256) void k_remap_fixed(rm_src S, const short* __restrict__ xy, const uint16_t* __restrict__ frac, int mw, int mh, int vec,
                                                     uint8_t* __restrict__ dst)
{
    int x0, y, n;
    if (!rm_lane(mw, mh, x0, y, n)) return;
    const size_t i0 = (size_t)y * mw + x0;
    int sx[RM_PPT], sy[RM_PPT], fr[RM_PPT];
    if (vec) {
        const uint4 q = *(const uint4*)(xy + 2 * i0);
        const u32 w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < RM_PPT; i++) { sx[i] = (short)(w[i] & 0xffffu); sy[i] = (short)(w[i] >> 16); }
        if (LINEAR) {
            const uint2 f = *(const uint2*)(frac + i0);
            fr[0] = f.x & 0xffffu; fr[1] = f.x >> 16; fr[2] = f.y & 0xffffu; fr[3] = f.y >> 16;
        }
    } else {
#pragma unroll
        for (int i = 0; i < RM_PPT; i++) {
            const bool on = i < n;
            sx[i] = on ? xy[2 * (i0 + i)] : 0;
            sy[i] = on ? xy[2 * (i0 + i) + 1] : 0;
            if (LINEAR) fr[i] = on ? frac[i0 + i] : 0;
        }
    }
    uint8_t o[RM_PPT * CN];
#pragma unroll
    for (int i = 0; i < RM_PPT; i++)
        if (i < n) rm_sample<CN, LINEAR>(S, sx[i], sy[i], LINEAR ? (fr[i] & 1023) : 0, o + i * CN);
    rm_store<CN>(dst + i0 * CN, o, vec != 0, n);
}

// The same gather from float maps: mapy != NULL: two planes; mapy == NULL: mapx holds interleaved (x, y) pairs.
template <int CN, bool LINEAR>
__global__ __launch_bounds__(256) void k_remap_f32(rm_src S, const float* __restrict__ mapx, const float* __restrict__ mapy, int mw, int mh, int vec,
                                                   uint8_t* __restrict__ dst)
{
    int x0, y, n;
    if (!rm_lane(mw, mh, x0, y, n)) return;
    const size_t i0 = (size_t)y * mw + x0;
    float mx[RM_PPT], my[RM_PPT];
    if (vec) {
        if (mapy) {
            const float4 a = *(const float4*)(mapx + i0), b = *(const float4*)(mapy + i0);
            mx[0] = a.x; mx[1] = a.y; mx[2] = a.z; mx[3] = a.w;
            my[0] = b.x; my[1] = b.y; my[2] = b.z; my[3] = b.w;
        } else {
            const float4 a = *(const float4*)(mapx + 2 * i0), b = *(const float4*)(mapx + 2 * i0 + 4);
            mx[0] = a.x; my[0] = a.y; mx[1] = a.z; my[1] = a.w;
            mx[2] = b.x; my[2] = b.y; mx[3] = b.z; my[3] = b.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < RM_PPT; i++) {
            const bool on = i < n;
            mx[i] = on ? (mapy ? mapx[i0 + i] : mapx[2 * (i0 + i)]) : 0.f;
            my[i] = on ? (mapy ? mapy[i0 + i] : mapx[2 * (i0 + i) + 1]) : 0.f;
        }
    }
    uint8_t o[RM_PPT * CN];
#pragma unroll
    for (int i = 0; i < RM_PPT; i++)
        if (i < n) {
            int sx, sy, fr;
            rm_convert<LINEAR>(mx[i], my[i], sx, sy, fr);
            rm_sample<CN, LINEAR>(S, sx, sy, fr, o + i * CN);
        }
    rm_store<CN>(dst + i0 * CN, o, vec != 0, n);
}

// cv2.convertMaps(float maps -> CV_16SC2 [+ CV_16UC1]): one entry per thread; frac == NULL with NEAREST
template <bool LINEAR>
__global__ __launch_bounds__(RM_CVT_BLOCK) void k_convert_maps(const float* __restrict__ mapx, const float* __restrict__ mapy, size_t n, short* __restrict__ xy,
                                                               uint16_t* __restrict__ frac)
{
    const size_t i = (size_t)blockIdx.x * RM_CVT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float mx = mapy ? mapx[i] : mapx[2 * i], my = mapy ? mapy[i] : mapx[2 * i + 1];
    int sx, sy, fr;
    rm_convert<LINEAR>(mx, my, sx, sy, fr);
    xy[2 * i] = (short)sx;                 // two 2-byte stores: xy_out need not be 4-byte aligned
    xy[2 * i + 1] = (short)sy;
    if (LINEAR) frac[i] = (uint16_t)fr;
}

// cv2.warpPerspective: m maps destination to source (the host inverts).  Columns are processed in blocks of bw0 as
// cv::WarpPerspectiveInvoker does, and the block origin is part of the rounding: X0 = M0 bx + M1 y + M2, then X0 + M0 (x - bx).
struct wp_params { double m[9]; int dw, dh, bw0; };
__device__ __forceinline__ int wp_round(double v)      // saturate_cast<int>(max(INT_MIN, min(INT_MAX, v))), std::min / std::max operand order
{
    double t = v < 2147483647.0 ? v : 2147483647.0;
    t = -2147483648.0 < t ? t : -2147483648.0;
    return (int)rint(t);
}
template <int CN, bool LINEAR>
__global__ __launch_bounds__(256) void k_warp_perspective(rm_src S, wp_params P, int vec, uint8_t* __restrict__ dst)
{
    int x0, y, n;
    if (!rm_lane(P.dw, P.dh, x0, y, n)) return;
    const size_t i0 = (size_t)y * P.dw + x0;
    const double dy = (double)y;
    uint8_t o[RM_PPT * CN];
#pragma unroll
    for (int i = 0; i < RM_PPT; i++)
        if (i < n) {
            const int x = x0 + i, bx = (x / P.bw0) * P.bw0;
            const double dbx = (double)bx, dx1 = (double)(x - bx);
            const double X0 = __dadd_rn(__dadd_rn(__dmul_rn(P.m[0], dbx), __dmul_rn(P.m[1], dy)), P.m[2]);
            const double Y0 = __dadd_rn(__dadd_rn(__dmul_rn(P.m[3], dbx), __dmul_rn(P.m[4], dy)), P.m[5]);
            const double W0 = __dadd_rn(__dadd_rn(__dmul_rn(P.m[6], dbx), __dmul_rn(P.m[7], dy)), P.m[8]);
            double W = __dadd_rn(W0, __dmul_rn(P.m[6], dx1));
            W = W != 0.0 ? __ddiv_rn(LINEAR ? 32.0 : 1.0, W) : 0.0;
            const int X = wp_round(__dmul_rn(__dadd_rn(X0, __dmul_rn(P.m[0], dx1)), W));
            const int Y = wp_round(__dmul_rn(__dadd_rn(Y0, __dmul_rn(P.m[3], dx1)), W));
            if (LINEAR) rm_sample<CN, true>(S, rm_sat16(X >> 5), rm_sat16(Y >> 5), (Y & 31) * 32 + (X & 31), o + i * CN);
            else rm_sample<CN, false>(S, rm_sat16(X), rm_sat16(Y), 0, o + i * CN);
        }
    rm_store<CN>(dst + i0 * CN, o, vec != 0, n);
}

static rm_src rm_make_src(const uint8_t* d_src, size_t sstride, int sw, int sh, int cn, int border, const uint8_t* cval)
{
    rm_src S;
    S.p = d_src; S.stride = sstride ? sstride : (size_t)sw * cn; S.w = sw; S.h = sh; S.border = border;
    for (int c = 0; c < 4; c++) S.cval[c] = (cval && c < cn) ? cval[c] : 0;   // border_value holds cn bytes
    return S;
}
static bool rm_aligned16(const void* a, const void* b = nullptr, const void* c = nullptr)
{
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

#define RM_LAUNCH(kernel, cn, linear, grid, ...)                                                                     \
    do {                                                                                                              \
        const dim3 blk(64, RM_TH);                                                                                    \
        switch ((cn) * 2 + ((linear) ? 1 : 0)) {                                                                      \
        case 2: hipLaunchKernelGGL((kernel<1, false>), grid, blk, 0, ctx->stream, __VA_ARGS__); break;                \
        case 3: hipLaunchKernelGGL((kernel<1, true>), grid, blk, 0, ctx->stream, __VA_ARGS__); break;                 \
        case 4: hipLaunchKernelGGL((kernel<2, false>), grid, blk, 0, ctx->stream, __VA_ARGS__); break;                \
        case 5: hipLaunchKernelGGL((kernel<2, true>), grid, blk, 0, ctx->stream, __VA_ARGS__); break;                 \
        case 6: hipLaunchKernelGGL((kernel<3, false>), grid, blk, 0, ctx->stream, __VA_ARGS__); break;                \
        case 7: hipLaunchKernelGGL((kernel<3, true>), grid, blk, 0, ctx->stream, __VA_ARGS__); break;                 \
        case 8: hipLaunchKernelGGL((kernel<4, false>), grid, blk, 0, ctx->stream, __VA_ARGS__); break;                \
        case 9: hipLaunchKernelGGL((kernel<4, true>), grid, blk, 0, ctx->stream, __VA_ARGS__); break;                 \
        default: return vp_fail(ctx, VP_ERR_INVALID, "remap: cn must be 1..4");                                       \
        }                                                                                                             \
    } while (0)

int vpk_remap_fixed(vp_ctx* ctx, const uint8_t* d_src, size_t sstride, int sw, int sh, int cn, const int16_t* d_xy, const uint16_t* d_frac, int mw, int mh,
                    int linear, int border, const uint8_t* cval, uint8_t* d_dst)
{
    if (!vp_remap_sizes_ok(sw, sh, cn, mw, mh) || (linear && !d_frac)) return vp_fail(ctx, VP_ERR_INVALID, "remap (fixed maps): sizes");
    const rm_src S = rm_make_src(d_src, sstride, sw, sh, cn, border, cval);
    const int vec = mw % RM_PPT == 0 && rm_aligned16(d_xy, d_frac, d_dst);
    const dim3 grid(vp_remap_grid_x(mw), vp_remap_grid_y(mh));
    vp_prof_scope ps(ctx, VPK_OTHER);
    RM_LAUNCH(k_remap_fixed, cn, linear, grid, S, (const short*)d_xy, d_frac, mw, mh, vec, d_dst);
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

int vpk_remap_f32(vp_ctx* ctx, const uint8_t* d_src, size_t sstride, int sw, int sh, int cn, const float* d_mapx, const float* d_mapy, int mw, int mh,
                  int linear, int border, const uint8_t* cval, uint8_t* d_dst)
{
    if (!vp_remap_sizes_ok(sw, sh, cn, mw, mh)) return vp_fail(ctx, VP_ERR_INVALID, "remap (float maps): sizes");
    const rm_src S = rm_make_src(d_src, sstride, sw, sh, cn, border, cval);
    const int vec = mw % RM_PPT == 0 && rm_aligned16(d_mapx, d_mapy, d_dst);
    const dim3 grid(vp_remap_grid_x(mw), vp_remap_grid_y(mh));
    vp_prof_scope ps(ctx, VPK_OTHER);
    RM_LAUNCH(k_remap_f32, cn, linear, grid, S, d_mapx, d_mapy, mw, mh, vec, d_dst);
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

int vpk_convert_maps(vp_ctx* ctx, const float* d_mapx, const float* d_mapy, int mw, int mh, int nearest, int16_t* d_xy, uint16_t* d_frac)
{
    if (!vp_remap_map_ok(mw, mh) || (!nearest && !d_frac)) return vp_fail(ctx, VP_ERR_INVALID, "convert maps: sizes");
    const size_t n = (size_t)mw * mh;
    const dim3 grid((unsigned)((n + RM_CVT_BLOCK - 1) / RM_CVT_BLOCK));
    vp_prof_scope ps(ctx, VPK_OTHER);
    if (nearest) hipLaunchKernelGGL(k_convert_maps<false>, grid, dim3(RM_CVT_BLOCK), 0, ctx->stream, d_mapx, d_mapy, n, (short*)d_xy, d_frac);
    else hipLaunchKernelGGL(k_convert_maps<true>, grid, dim3(RM_CVT_BLOCK), 0, ctx->stream, d_mapx, d_mapy, n, (short*)d_xy, d_frac);
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

// cv::invert of a 3x3 double matrix (DECOMP_LU takes the closed form): the determinant by cofactors, d = 1 / det, each cofactor
// times d; a singular matrix gives zeros.  Plain IEEE double, no fused multiply-add.
void vp_invert33(const double* S, double* t)
{
#pragma clang fp contract(off)
    double d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
    if (d == 0.) {
        for (int i = 0; i < 9; i++) t[i] = 0.;
        return;
    }
    d = 1. / d;
    t[0] = (S[4] * S[8] - S[5] * S[7]) * d;
    t[1] = (S[2] * S[7] - S[1] * S[8]) * d;
    t[2] = (S[1] * S[5] - S[2] * S[4]) * d;
    t[3] = (S[5] * S[6] - S[3] * S[8]) * d;
    t[4] = (S[0] * S[8] - S[2] * S[6]) * d;
    t[5] = (S[2] * S[3] - S[0] * S[5]) * d;
    t[6] = (S[3] * S[7] - S[4] * S[6]) * d;
    t[7] = (S[1] * S[6] - S[0] * S[7]) * d;
    t[8] = (S[0] * S[4] - S[1] * S[3]) * d;
}

int vpk_warp_perspective(vp_ctx* ctx, const uint8_t* d_src, size_t sstride, int sw, int sh, int cn, const double* M33, int inverse_map, int linear, int border,
                         const uint8_t* cval, uint8_t* d_dst, int dw, int dh)
{
    if (!vp_remap_sizes_ok(sw, sh, cn, dw, dh)) return vp_fail(ctx, VP_ERR_INVALID, "warp perspective: sizes");
    const rm_src S = rm_make_src(d_src, sstride, sw, sh, cn, border, cval);
    wp_params P;
    if (inverse_map) for (int i = 0; i < 9; i++) P.m[i] = M33[i];
    else vp_invert33(M33, P.m);
    P.dw = dw; P.dh = dh; P.bw0 = vp_wp_block_width(dw, dh);
    const int vec = dw % RM_PPT == 0 && rm_aligned16(d_dst);
    const dim3 grid(vp_remap_grid_x(dw), vp_remap_grid_y(dh));
    vp_prof_scope ps(ctx, VPK_OTHER);
    RM_LAUNCH(k_warp_perspective, cn, linear, grid, S, P, vec, d_dst);
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
