// cv2.cornerMinEigenVal / cv2.cornerHarris / cv2.goodFeaturesToTrack on uint8 single-channel images, gradient size 3 (DESIGN.md
// section 4.24; tests/corners_restate.py is the statement).  OpenCV runs the structure tensor through float32 SIMD code whose rounding
// cannot be restated; what it approximates is restated here exactly.  For a uint8 image the Sobel taps, their products and the
// blockSize x blockSize box sums are integers below 2^31 (vp_corners_plan.h), and only the eigenvalue formula is floating point: IEEE
// double, a fixed operation order, no contraction, one rounding to float32.
//
//   k_corner_response<HB, HARRIS>  one pass, a block of 256 threads per CR_TW x CR_TH tile of results, blockSize B <= HB:
//     1. stages the source tile and a halo of 1 + B / 2 + 1 pixels in LDS, the border applied (vp_deriv_border_index);
//     2. forms (Dx, Dy) once per pixel of the tile and its box halo as an int16 pair.  The box sums apply the border to the PRODUCT
//        image, as cornerEigenValsVecs does when it runs boxFilter on `cov`: a halo pixel outside the image is the product pixel the
//        border maps it to, whose own Sobel window is read from the image (only tiles at the image's edge have such pixels);
//     3. row sums of Dx Dx, Dx Dy, Dy Dy by a sliding window, CR_SEG results per thread, three int32 planes in LDS;
//     4. column sums the same way, four rows per thread, then the response in double and one float32 store per result, 256 contiguous
//        bytes per wave.
//   k_corner_max     block maximum of the response over the pixels the mask admits (bytes, or a bit plane), one atomic per block on
//                    the float's order-preserving integer key (Harris responses can be negative).
//   k_corner_cand    threshold t = (float)((double)max * quality) from that word, the 3 x 3 test, candidates appended as 64-bit words by
//                    a ballot per wave and one atomic per block.
//   vpk_hough_sort_keys orders the words; the greedy minDistance pass is host code (vp_good_features_select).
#include "vp_internal.h"
#include "vp_corners_plan.h"

static_assert(VP_DV_CONSTANT == VP_BORDER_CONSTANT && VP_DV_REPLICATE == VP_BORDER_REPLICATE && VP_DV_REFLECT == VP_BORDER_REFLECT &&
              VP_DV_REFLECT_101 == VP_BORDER_REFLECT_101, "border codes of vp.h");

namespace {

template <int HB>
struct cr_tile {
    static constexpr int PW = CR_TW + HB - 1;          // product pixels per staged row: the tile and its box halo
    static constexpr int PH = CR_TH + HB - 1;
    static constexpr int SP = (PW + 2 + 3) & ~3;       // source bytes per staged row: one more pixel each side for the Sobel
    static constexpr int DP = PW | 1;                  // odd pitches: a wave walks rows of D and writes rows of the sums without bank conflicts
    static constexpr int RP = CR_TW + 1;
    static constexpr int LDS = (PH + 2) * SP + PH * DP * 4 + 3 * PH * RP * 4;
};
static_assert(cr_tile<CR_MAX_BLOCK>::LDS <= 64 * 1024, "k_corner_response: static LDS above 64 KiB");

__device__ __forceinline__ int cr_dx(u32 v) { return (int)(short)(v & 0xffffu); }
__device__ __forceinline__ int cr_dy(u32 v) { return (int)v >> 16; }

// pixel (x, y) of the border-extended source, however far outside the image; 0 beyond a constant border
__device__ __forceinline__ int cr_src(const uint8_t* __restrict__ src, size_t stride, int w, int h, int border, int x, int y)
{
    const int xx = vp_deriv_border_index(x, w, border), yy = vp_deriv_border_index(y, h, border);
    return (xx < 0 || yy < 0) ? 0 : (int)src[(size_t)yy * stride + xx];
}

// grid (ceil(w / CR_TW), ceil(h / CR_TH)), 256 threads.  ss: s * s (HARRIS: (s * s) * (s * s)), s of vp_corner_scale; dst packed.
template <int HB, bool HARRIS>
__global__ __launch_bounds__(256) void k_corner_response(const uint8_t* __restrict__ src, size_t stride, int w, int h, int B, int border, double k, double ss,
                                                         float* __restrict__ dst)
{
    typedef cr_tile<HB> T;
    __shared__ uint8_t S[(T::PH + 2) * T::SP];
    __shared__ u32 D[T::PH * T::DP];
    __shared__ int RS[3][T::PH * T::RP];
    const int a = B / 2;
    const int x0 = blockIdx.x * CR_TW, y0 = blockIdx.y * CR_TH;
    const int tw = min(CR_TW, w - x0), th = min(CR_TH, h - y0);
    const int pw = tw + B - 1, ph = th + B - 1;        // product pixels staged: columns x0 - a .., rows y0 - a ..
    // 1. the source under its border, columns x0 - a - 1 .., rows y0 - a - 1 ..
    for (int i = threadIdx.x; i < (ph + 2) * (pw + 2); i += 256) {
        const int j = i / (pw + 2), c = i - j * (pw + 2);
        S[j * T::SP + c] = (uint8_t)cr_src(src, stride, w, h, border, x0 - a - 1 + c, y0 - a - 1 + j);
    }
    __syncthreads();
    // 2. the Sobel pair of every staged product pixel
    for (int i = threadIdx.x; i < ph * pw; i += 256) {
        const int j = i / pw, c = i - j * pw;
        const int ex = x0 - a + c, ey = y0 - a + j;
        int dx, dy;
        if ((unsigned)ex < (unsigned)w && (unsigned)ey < (unsigned)h) {
            const uint8_t* p = S + j * T::SP + c;                  // the window's upper left pixel
            const int p00 = p[0], p01 = p[1], p02 = p[2], p10 = p[T::SP], p12 = p[T::SP + 2], p20 = p[2 * T::SP], p21 = p[2 * T::SP + 1],
                      p22 = p[2 * T::SP + 2];
            dx = (p02 + 2 * p12 + p22) - (p00 + 2 * p10 + p20);
            dy = (p20 + 2 * p21 + p22) - (p00 + 2 * p01 + p02);
        } else {
            const int mx = vp_deriv_border_index(ex, w, border), my = vp_deriv_border_index(ey, h, border);
            dx = dy = 0;                                           // beyond a constant border the product is 0
            if (mx >= 0 && my >= 0) {
                const int p00 = cr_src(src, stride, w, h, border, mx - 1, my - 1), p01 = cr_src(src, stride, w, h, border, mx, my - 1),
                          p02 = cr_src(src, stride, w, h, border, mx + 1, my - 1), p10 = cr_src(src, stride, w, h, border, mx - 1, my),
                          p12 = cr_src(src, stride, w, h, border, mx + 1, my), p20 = cr_src(src, stride, w, h, border, mx - 1, my + 1),
                          p21 = cr_src(src, stride, w, h, border, mx, my + 1), p22 = cr_src(src, stride, w, h, border, mx + 1, my + 1);
                dx = (p02 + 2 * p12 + p22) - (p00 + 2 * p10 + p20);
                dy = (p20 + 2 * p21 + p22) - (p00 + 2 * p01 + p02);
            }
        }
        D[j * T::DP + c] = ((u32)dx & 0xffffu) | ((u32)dy << 16);
    }
    __syncthreads();
    // 3. row sums: staged row j, results c0 .. c0 + CR_SEG - 1; neighbouring lanes take neighbouring rows
    const int nseg = (tw + CR_SEG - 1) / CR_SEG;
    for (int i = threadIdx.x; i < ph * nseg; i += 256) {
        const int seg = i / ph, j = i - seg * ph;
        const int c0 = seg * CR_SEG, c1 = min(c0 + CR_SEG, tw);
        const u32* d = D + j * T::DP;
        int xx = 0, xy = 0, yy = 0;
        for (int t = c0; t < c0 + B; t++) {
            const int gx = cr_dx(d[t]), gy = cr_dy(d[t]);
            xx += gx * gx; xy += gx * gy; yy += gy * gy;
        }
        for (int c = c0;; c++) {
            RS[0][j * T::RP + c] = xx;
            RS[1][j * T::RP + c] = xy;
            RS[2][j * T::RP + c] = yy;
            if (c + 1 >= c1) break;
            const int ax = cr_dx(d[c + B]), ay = cr_dy(d[c + B]), sx = cr_dx(d[c]), sy = cr_dy(d[c]);
            xx += ax * ax - sx * sx; xy += ax * ay - sx * sy; yy += ay * ay - sy * sy;
        }
    }
    __syncthreads();
    // 4. column sums and the response: lane = column, four rows per thread
    const int c = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * (CR_TH / 4), r1 = min(r0 + CR_TH / 4, th);
    if (c >= tw || r0 >= r1) return;
    int sxx = 0, sxy = 0, syy = 0;
    for (int j = r0; j < r0 + B; j++) {
        sxx += RS[0][j * T::RP + c]; sxy += RS[1][j * T::RP + c]; syy += RS[2][j * T::RP + c];
    }
    for (int r = r0;; r++) {
        double resp;
        if (HARRIS) {
            const double A = (double)sxx, Bm = (double)sxy, C = (double)syy;
            const double H = (A * C - Bm * Bm) - k * ((A + C) * (A + C));
            resp = H * ss;
        } else {
            const double A = (double)sxx * 0.5, Bm = (double)sxy, C = (double)syy * 0.5;
            const double L = (A + C) - __dsqrt_rn((A - C) * (A - C) + Bm * Bm);
            resp = L * ss;
        }
        dst[(size_t)(y0 + r) * w + x0 + c] = (float)resp;
        if (r + 1 >= r1) break;
        sxx += RS[0][(r + B) * T::RP + c] - RS[0][r * T::RP + c];
        sxy += RS[1][(r + B) * T::RP + c] - RS[1][r * T::RP + c];
        syy += RS[2][(r + B) * T::RP + c] - RS[2][r * T::RP + c];
    }
}

template <int HB>
void cr_launch(vp_ctx* ctx, dim3 grid, const uint8_t* src, size_t stride, int w, int h, int B, int border, int harris, double k, float* dst)
{
    const double s = vp_corner_scale(B), ss = s * s;
    if (harris) hipLaunchKernelGGL((k_corner_response<HB, true>), grid, dim3(256), 0, ctx->stream, src, stride, w, h, B, border, k, ss * ss, dst);
    else hipLaunchKernelGGL((k_corner_response<HB, false>), grid, dim3(256), 0, ctx->stream, src, stride, w, h, B, border, k, ss, dst);
}

__device__ __forceinline__ bool cr_masked_in(const uint8_t* __restrict__ mask, size_t mstride, const u64* __restrict__ bits, int ww, int x, int y)
{
    if (bits) return (bits[(size_t)y * ww + (x >> 6)] >> (x & 63)) & 1ull;
    return !mask || mask[(size_t)y * mstride + x] != 0;
}

// grid min(ceil(w * h / 256), 2048), 256 threads: *out = max(*out, key of the largest admitted response); 0 = no pixel admitted
__global__ __launch_bounds__(256) void k_corner_max(const float* __restrict__ resp, int w, int h, const uint8_t* __restrict__ mask, size_t mstride,
                                                    const u64* __restrict__ bits, int ww, u32* __restrict__ out)
{
    __shared__ u32 part[4];
    const size_t npx = (size_t)w * h;
    u32 best = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npx; i += (size_t)gridDim.x * 256) {
        const int y = (int)(i / (unsigned)w), x = (int)(i - (size_t)y * w);
        if (cr_masked_in(mask, mstride, bits, ww, x, y)) best = max(best, vp_corner_key(__float_as_uint(resp[i])));
    }
    for (int off = 32; off; off >>= 1) best = max(best, (u32)__shfl_xor((int)best, off));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        best = max(max(part[0], part[1]), max(part[2], part[3]));
        if (best) atomicMax(out, best);
    }
}

// grid ceil(w * h / 256), 256 threads.  cnt[0]: the maximum's key (k_corner_max); cnt[1]: candidates appended so far.  A candidate:
// interior, above t, not 0, not below any of its eight neighbours that is above t, admitted by the mask.
__global__ __launch_bounds__(256) void k_corner_cand(const float* __restrict__ resp, int w, int h, const uint8_t* __restrict__ mask, size_t mstride,
                                                     const u64* __restrict__ bits, int ww, double quality, u32* __restrict__ cnt, u64* __restrict__ keys,
                                                     size_t kcap)
{
    __shared__ u32 wsum[4], wbase[4];
    const u32 mkey = cnt[0];
    const size_t npx = (size_t)w * h;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool pk = false;
    float v = 0.f;
    if (mkey != 0 && i < npx) {
        const float t = (float)((double)__uint_as_float(vp_corner_unkey(mkey)) * quality);
        const int y = (int)(i / (unsigned)w), x = (int)(i - (size_t)y * w);
        if (x >= 1 && y >= 1 && x <= w - 2 && y <= h - 2) {
            v = resp[i];
            if (v > t && v != 0.f && cr_masked_in(mask, mstride, bits, ww, x, y)) {
                pk = true;
#pragma unroll
                for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                    for (int dx = -1; dx <= 1; dx++) {
                        const float n = resp[i + (ptrdiff_t)dy * w + dx];
                        if (n > t && n > v) pk = false;
                    }
            }
        }
    }
    const u64 m = __ballot(pk);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wsum[wave] = (u32)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        const u32 tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        u32 b = tot ? atomicAdd(&cnt[1], tot) : 0;
        for (int q = 0; q < 4; q++) { wbase[q] = b; b += wsum[q]; }
    }
    __syncthreads();
    if (pk) {
        const size_t pos = (size_t)wbase[wave] + __popcll(m & ((1ull << lane) - 1ull));
        if (pos < kcap) keys[pos] = ~(((u64)vp_corner_key(__float_as_uint(v)) << 32) | (u64)(u32)i);
    }
}

}  // namespace

// arguments as vp_corner_response_refusal admitted them; d_dst: w * h floats, packed; one launch, enqueued
int vpk_corner_response(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int block_size, int harris, double k, int border, float* d_dst)
{
    vp_prof_scope ps(ctx, VPK_OTHER);
    const dim3 grid((unsigned)((w + CR_TW - 1) / CR_TW), (unsigned)((h + CR_TH - 1) / CR_TH));
    border &= ~VP_DV_ISOLATED;
    switch (vp_corner_block_class(block_size)) {
        case 3: cr_launch<3>(ctx, grid, d_src, stride, w, h, block_size, border, harris, k, d_dst); break;
        case 7: cr_launch<7>(ctx, grid, d_src, stride, w, h, block_size, border, harris, k, d_dst); break;
        default: cr_launch<CR_MAX_BLOCK>(ctx, grid, d_src, stride, w, h, block_size, border, harris, k, d_dst); break;
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

// d_cnt: two words, zeroed here: the maximum's key and the candidate count; d_keys: kcap words, the first min(count, kcap) written in
// no particular order.  d_mask (nullable, rows of mstride bytes) or d_bits (nullable, its bit plane) admit pixels.  Two launches, enqueued.
int vpk_corner_candidates(vp_ctx* ctx, const float* d_resp, int w, int h, const uint8_t* d_mask, size_t mstride, const u64* d_bits, double quality,
                          u32* d_cnt, u64* d_keys, size_t kcap)
{
    const size_t npx = (size_t)w * h;
    const int ww = vp_ww(w);
    VP_HIP(ctx, hipMemsetAsync(d_cnt, 0, 8, ctx->stream));
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_corner_max, dim3((unsigned)((npx + 255) / 256 < 2048 ? (npx + 255) / 256 : 2048)), dim3(256), 0, ctx->stream, d_resp, w, h, d_mask,
                           mstride, d_bits, ww, d_cnt);
    }
    VP_HIP(ctx, hipGetLastError());
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_corner_cand, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, ctx->stream, d_resp, w, h, d_mask, mstride, d_bits, ww, quality,
                           d_cnt, d_keys, kcap);
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
