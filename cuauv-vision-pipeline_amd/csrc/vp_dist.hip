// cv2.distanceTransform (DIST_L2 with DIST_MASK_PRECISE, DIST_L1, DIST_C) and cv2.minMaxLoc (DESIGN.md section 4.25;
// tests/dist_restate.py is the statement).  Zero pixels are the sources.  All three metrics separate into a row pass and a column pass
// over exact integers, and only the last step of DIST_L2 is floating point: the correctly rounded float32 root of float32(D2).
//
//   k_dist_rows   one wave per row, one 64-bit word of the row per lane (w <= 4096).  The words come from the mask's bit plane, or are
//                 made from its bytes by ballot; bits past w count as non-zero pixels whatever the plane holds there.  A prefix maximum
//                 of "last zero at or before this word" and a suffix minimum of "first zero at or after it" over the wave give every
//                 word its carries, clz / ctz on the masked zero bits finish each pixel: g(x, y), the horizontal distance to the nearest
//                 zero of row y, uint16, DT_NONE where the row has none.  Rows of g are padded to whole words and the padding is DT_NONE.
//   k_dist_cols   D(x, y) = min over y' of cost(|y - y'|, g(x, y')), cost = dy^2 + g^2, dy + g or max(dy, g).  Each lane owns four
//                 neighbouring pixels of a row and searches outwards, dy = 1, 2, ..., until dy^2 (dy for L1 and C) reaches the best cost
//                 of its four, at most max(y, h - 1 - y) steps: no loop depends on anything but h.  Two forms (vp_dist_plan.h picks):
//                 STAGED keeps all h rows of a strip of DT_STRIP_COLS columns of g in LDS (h <= DT_STAGED_MAX_H), the other reads g from
//                 device memory.  A cost at or above DT_NONE's is +inf (255 for CV_8U): the image has no zero.
//   k_min_max_loc grid-stride search for both ends at once: per lane, per wave by shuffles, then one pair of 64-bit atomic maxima per
//                 block on the keys of vp_dist_plan.h (ties to the smallest raster index at both ends; NaN and masked pixels take no part).
#include "vp_internal.h"
#include "vp_dist_plan.h"

static_assert(DT_DEPTH_8U == VP_DEPTH_8U && DT_DEPTH_32F == VP_DEPTH_32F && DT_METRIC_L1 == VP_DIST_L1 && DT_METRIC_L2 == VP_DIST_L2 && DT_METRIC_C == VP_DIST_C,
              "depth and metric codes of vp.h");

namespace {

#define DT_FAR (1 << 20)       // "no zero on this side": further than any pixel, small enough to subtract in int

// grid ceil(h / DT_ROW_WAVES), 64 * DT_ROW_WAVES threads.  bits (nullable): rows of ww words; src: rows of stride bytes, read only
// when bits is null.  g: rows of gp = 64 * ww uint16.
__global__ __launch_bounds__(64 * DT_ROW_WAVES) void k_dist_rows(const uint8_t* __restrict__ src, size_t stride, const u64* __restrict__ bits, int ww, int w,
                                                                 int h, uint16_t* __restrict__ g, int gp)
{
    const int lane = threadIdx.x & 63, y = blockIdx.x * DT_ROW_WAVES + (threadIdx.x >> 6);
    if (y >= h) return;                                 // whole waves leave: nothing below synchronises the block
    u64 nz = 0;
    if (bits) {
        if (lane < ww) nz = bits[(size_t)y * ww + lane];
    } else {
        for (int k = 0; k < ww; k++) {
            const int x = 64 * k + lane;
            const u64 m = __ballot(x < w && src[(size_t)y * stride + x] != 0);
            if (lane == k) nz = m;
        }
    }
    const int nvalid = min(max(w - 64 * lane, 0), 64);
    const u64 z = ~nz & (nvalid == 64 ? ~0ull : ((1ull << nvalid) - 1ull));     // the zero pixels of this lane's word
    int last = z ? 64 * lane + 63 - __clzll((long long)z) : -DT_FAR;
    int first = z ? 64 * lane + (__ffsll((long long)z) - 1) : DT_FAR;
    for (int off = 1; off < 64; off <<= 1) {
        const int a = __shfl_up(last, off), b = __shfl_down(first, off);
        if (lane >= off) last = max(last, a);
        if (lane + off < 64) first = min(first, b);
    }
    for (int k = 0; k < ww; k++) {
        const u64 zk = __shfl(z, k);
        const int lc = __shfl(last, k > 0 ? k - 1 : 0), rc = __shfl(first, k < 63 ? k + 1 : 63);
        const int x = 64 * k + lane;
        const u64 le = zk & (~0ull >> (63 - lane)), ge = zk & (~0ull << lane);
        const int l = le ? 64 * k + 63 - __clzll((long long)le) : (k > 0 ? lc : -DT_FAR);
        const int r = ge ? 64 * k + (__ffsll((long long)ge) - 1) : (k < 63 ? rc : DT_FAR);
        const int d = x < w ? min(min(x - l, r - x), DT_NONE) : DT_NONE;
        g[(size_t)y * gp + x] = (uint16_t)d;
    }
}

template <int METRIC>
__device__ __forceinline__ int dt_cost(int dy, int gv)
{
    if (METRIC == VP_DIST_L2) return dy * dy + gv * gv;
    if (METRIC == VP_DIST_L1) return dy + gv;
    return max(dy, gv);
}

template <int METRIC>
__device__ __forceinline__ void dt_take(uint2 v, int dy, int& b0, int& b1, int& b2, int& b3)
{
    b0 = min(b0, dt_cost<METRIC>(dy, (int)(v.x & 0xffffu)));
    b1 = min(b1, dt_cost<METRIC>(dy, (int)(v.x >> 16)));
    b2 = min(b2, dt_cost<METRIC>(dy, (int)(v.y & 0xffffu)));
    b3 = min(b3, dt_cost<METRIC>(dy, (int)(v.y >> 16)));
}

// The float32 root goes through the double root, which is correctly rounded on this device (the corner kernels rely on it too), and
// rounding a 53-bit root of a 24-bit argument to 24 bits is the correctly rounded float32 root (53 >= 2 * 24 + 2).  __fsqrt_rn is the
// hardware's approximate root here: it was one ulp off at sqrt(82).
template <int METRIC>
__device__ __forceinline__ float dt_value(int best)
{
    if (METRIC == VP_DIST_L2) return best >= DT_NONE * DT_NONE ? __builtin_inff() : (float)__dsqrt_rn((double)(float)best);
    return best >= DT_NONE ? __builtin_inff() : (float)best;
}

// grid vp_dist_grid, 256 threads, STAGED: vp_dist_lds_bytes(h) of dynamic LDS.  dst: rows of dstride bytes, float32 or (depth8) uint8;
// vec: dst and dstride allow one aligned store of the lane's four results.
template <int METRIC, bool STAGED>
__global__ __launch_bounds__(256) void k_dist_cols(const uint16_t* __restrict__ g, int gp, int w, int h, int depth8, int vec, uint8_t* __restrict__ dst,
                                                   size_t dstride)
{
    constexpr int COLS = STAGED ? DT_STRIP_COLS : DT_WIDE_COLS, ROWS = STAGED ? DT_STRIP_ROWS : DT_WIDE_ROWS;
    constexpr int LPR = COLS / DT_PX, RPP = 256 / LPR;          // lanes per row of the block, rows per pass
    extern __shared__ uint2 S[];                                // STAGED: h rows of LPR words, four uint16 each
    const int x0 = blockIdx.x * COLS, y0 = blockIdx.y * ROWS;
    if (STAGED) {
        for (int i = threadIdx.x; i < h * LPR; i += 256) {
            const int r = i / LPR, c = i - r * LPR;
            S[i] = *reinterpret_cast<const uint2*>(g + (size_t)r * gp + x0 + c * DT_PX);
        }
        __syncthreads();
    }
    const int c = threadIdx.x % LPR, x = x0 + c * DT_PX;
    if (x >= w) return;
    const uint16_t* gc = g + x;
    for (int pass = 0; pass < ROWS / RPP; pass++) {
        const int y = y0 + pass * RPP + threadIdx.x / LPR;
        if (y >= h) break;
        uint2 v = STAGED ? S[y * LPR + c] : *reinterpret_cast<const uint2*>(gc + (size_t)y * gp);
        int b0 = dt_cost<METRIC>(0, (int)(v.x & 0xffffu));
        int b1 = x + 1 < w ? dt_cost<METRIC>(0, (int)(v.x >> 16)) : 0;       // a pixel past the row never prolongs the search
        int b2 = x + 2 < w ? dt_cost<METRIC>(0, (int)(v.y & 0xffffu)) : 0;
        int b3 = x + 3 < w ? dt_cost<METRIC>(0, (int)(v.y >> 16)) : 0;
        const int lim = max(y, h - 1 - y);
        for (int dy = 1; dy <= lim; dy++) {
            if ((METRIC == VP_DIST_L2 ? dy * dy : dy) >= max(max(b0, b1), max(b2, b3))) break;
            if (y - dy >= 0) {
                v = STAGED ? S[(y - dy) * LPR + c] : *reinterpret_cast<const uint2*>(gc + (size_t)(y - dy) * gp);
                dt_take<METRIC>(v, dy, b0, b1, b2, b3);
            }
            if (y + dy < h) {
                v = STAGED ? S[(y + dy) * LPR + c] : *reinterpret_cast<const uint2*>(gc + (size_t)(y + dy) * gp);
                dt_take<METRIC>(v, dy, b0, b1, b2, b3);
            }
        }
        uint8_t* row = dst + (size_t)y * dstride;
        if (depth8) {
            const u32 q0 = (u32)min(b0, 255), q1 = (u32)min(b1, 255), q2 = (u32)min(b2, 255), q3 = (u32)min(b3, 255);
            if (vec && x + 3 < w) {
                *reinterpret_cast<u32*>(row + x) = q0 | (q1 << 8) | (q2 << 16) | (q3 << 24);
            } else {
                row[x] = (uint8_t)q0;
                if (x + 1 < w) row[x + 1] = (uint8_t)q1;
                if (x + 2 < w) row[x + 2] = (uint8_t)q2;
                if (x + 3 < w) row[x + 3] = (uint8_t)q3;
            }
        } else {
            float* frow = reinterpret_cast<float*>(row);
            const float f0 = dt_value<METRIC>(b0), f1 = dt_value<METRIC>(b1), f2 = dt_value<METRIC>(b2), f3 = dt_value<METRIC>(b3);
            if (vec && x + 3 < w) {
                *reinterpret_cast<float4*>(frow + x) = make_float4(f0, f1, f2, f3);
            } else {
                frow[x] = f0;
                if (x + 1 < w) frow[x + 1] = f1;
                if (x + 2 < w) frow[x + 2] = f2;
                if (x + 3 < w) frow[x + 3] = f3;
            }
        }
    }
}

template <int METRIC>
void dt_launch_cols(vp_ctx* ctx, const uint16_t* g, int gp, int w, int h, int depth8, int vec, uint8_t* dst, size_t dstride)
{
    unsigned gx, gy;
    vp_dist_grid(w, h, &gx, &gy);
    if (vp_dist_staged(h))
        hipLaunchKernelGGL((k_dist_cols<METRIC, true>), dim3(gx, gy), dim3(256), vp_dist_lds_bytes(h), ctx->stream, g, gp, w, h, depth8, vec, dst, dstride);
    else
        hipLaunchKernelGGL((k_dist_cols<METRIC, false>), dim3(gx, gy), dim3(256), 0, ctx->stream, g, gp, w, h, depth8, vec, dst, dstride);
}

__device__ __forceinline__ u64 mml_shfl_xor(u64 v, int off)
{
    const u32 lo = (u32)__shfl_xor((int)(u32)v, off), hi = (u32)__shfl_xor((int)(u32)(v >> 32), off);
    return ((u64)hi << 32) | lo;
}

// grid min(ceil(w * h / 256), 2048), 256 threads.  out[0]: the minimum's key, out[1]: the maximum's, both zeroed by the caller.
// mask (nullable, rows of mstride bytes) or mbits (nullable, its bit plane, rows of ww words) admit pixels.
__global__ __launch_bounds__(256) void k_min_max_loc(const uint8_t* __restrict__ src, size_t stride, int w, int h, int depth8, const uint8_t* __restrict__ mask,
                                                     size_t mstride, const u64* __restrict__ mbits, int ww, u64* __restrict__ out)
{
    __shared__ u64 part[2][4];
    const size_t npx = (size_t)w * h;
    u64 kmin = 0, kmax = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npx; i += (size_t)gridDim.x * 256) {
        const int y = (int)(i / (unsigned)w), x = (int)(i - (size_t)y * w);
        if (mbits) {
            if (!((mbits[(size_t)y * ww + (x >> 6)] >> (x & 63)) & 1ull)) continue;
        } else if (mask && mask[(size_t)y * mstride + x] == 0) continue;
        float v = depth8 ? (float)src[(size_t)y * stride + x] : *reinterpret_cast<const float*>(src + (size_t)y * stride + (size_t)x * 4);
        if (v != v) continue;                           // NaN takes no part
        v += 0.0f;                                      // -0 and +0 are one value, as in every comparison
        const u32 vb = __float_as_uint(v);
        kmin = max(kmin, (u64)vp_mml_key(vb, (u32)i, 1));
        kmax = max(kmax, (u64)vp_mml_key(vb, (u32)i, 0));
    }
    for (int off = 32; off; off >>= 1) {
        kmin = max(kmin, mml_shfl_xor(kmin, off));
        kmax = max(kmax, mml_shfl_xor(kmax, off));
    }
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = kmin;
        part[1][threadIdx.x >> 6] = kmax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        kmin = max(max(part[0][0], part[0][1]), max(part[0][2], part[0][3]));
        kmax = max(max(part[1][0], part[1][1]), max(part[1][2], part[1][3]));
        if (kmin) atomicMax(&out[0], kmin);
        if (kmax) atomicMax(&out[1], kmax);
    }
}

}  // namespace

// arguments as vp_distance_transform_refusal admitted them; d_bits (nullable): the source's bit plane, read instead of its bytes;
// d_g: vp_dist_g_bytes(w, h) of workspace; d_dst: rows of dstride bytes.  Two launches, enqueued.
int vpk_distance_transform(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, const u64* d_bits, int metric, int depth, uint16_t* d_g, void* d_dst,
                           size_t dstride)
{
    const int ww = vp_ww(w), gp = vp_dist_g_pitch(w);
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_dist_rows, dim3((unsigned)((h + DT_ROW_WAVES - 1) / DT_ROW_WAVES)), dim3(64 * DT_ROW_WAVES), 0, ctx->stream, d_src, stride, d_bits, ww, w,
                           h, d_g, gp);
    }
    VP_HIP(ctx, hipGetLastError());
    const int depth8 = depth == VP_DEPTH_8U;
    const size_t va = depth8 ? 4 : 16;
    const int vec = (uintptr_t)d_dst % va == 0 && dstride % va == 0;
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        switch (metric) {
            case VP_DIST_L2: dt_launch_cols<VP_DIST_L2>(ctx, d_g, gp, w, h, depth8, vec, (uint8_t*)d_dst, dstride); break;
            case VP_DIST_L1: dt_launch_cols<VP_DIST_L1>(ctx, d_g, gp, w, h, depth8, vec, (uint8_t*)d_dst, dstride); break;
            default: dt_launch_cols<VP_DIST_C>(ctx, d_g, gp, w, h, depth8, vec, (uint8_t*)d_dst, dstride); break;
        }
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

// arguments as vp_min_max_loc_refusal admitted them; d_out: two words, zeroed here, then the keys of the minimum and the maximum
// (vp_min_max_loc_decode).  One launch behind the zeroing, enqueued.
int vpk_min_max_loc(vp_ctx* ctx, const void* d_src, size_t stride, int w, int h, int depth, const uint8_t* d_mask, size_t mstride, const u64* d_mbits, u64* d_out)
{
    const size_t npx = (size_t)w * h;
    VP_HIP(ctx, hipMemsetAsync(d_out, 0, 16, ctx->stream));
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_min_max_loc, dim3((unsigned)((npx + 255) / 256 < 2048 ? (npx + 255) / 256 : 2048)), dim3(256), 0, ctx->stream, (const uint8_t*)d_src,
                           stride, w, h, depth == VP_DEPTH_8U, d_mask, mstride, d_mbits, vp_ww(w), d_out);
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
