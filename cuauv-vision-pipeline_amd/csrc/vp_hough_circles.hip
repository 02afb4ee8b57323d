// cv2.HoughCircles(image, HOUGH_GRADIENT, dp, minDist, None, param1, param2, minRadius, maxRadius) (utils/feature.py:128-155
// `find_circles`): OpenCV 4.x HoughCircles -> HoughCirclesGradient with maxRadius >= 0 and no cap on the number of circles.
//
// What is reproduced (imgproc/src/hough.cpp), all float arithmetic in float32 with every operation rounded on its own:
//   dp = max((float)dp, 1), idp = 1 / dp; edges = Canny(image, max(1, cvRound(param1) / 2), cvRound(param1)), 3x3, L1; dx, dy = the
//   CV_16S Sobel with BORDER_REPLICATE (the Canny's own derivatives);
//   an edge pixel (x, y) with (dx, dy) != 0 joins the point set; sx = cvRound(dx * idp * 1024 / |g|), x0 = cvRound(x * idp * 1024)
//   (y likewise); for each sign of (sx, sy) and r = minRadius .. maxRadius the cell ((x0 + r sx) >> 10, (y0 + r sy) >> 10) of the
//   cvCeil(rows * idp) x cvCeil(cols * idp) accumulator gets a vote, stopping at the first cell outside;
//   a centre is a cell above cvRound(param2), above its left and upper neighbours and not below its right and lower ones, ordered by
//   votes descending then bordered offset ascending (hough_cmp_gt);
//   per centre, the distances sqrt(r2) of the points with minR^2 <= r2 <= maxR^2 are binned by cvRound((d - minR) / dp * 10) and the
//   groups of ten bins walked from the top (HoughCircleEstimateRadiusInvoker, point-list form); a circle needs support > cvRound(param2);
//   circles are ordered by support, radius descending, x, y ascending (cmpAccum) and kept greedily at >= minDist from every kept one.
// Votes and histograms are integer counts and every float step is a scalar IEEE operation, so the order in which the GPU does the work
// does not change a bit of the result.
//
// Steps (one image, the context's stream):
//   vpk_canny_u8      edges and the Sobel plane (d_grad)
//   k_hc_points       edge pixels with a gradient -> rays (x0, y0, sx, sy) and the last r of each sign's run, one atomic per block
//   k_hc_vote         one block per 128 x 64 tile of the bordered accumulator: each ray's r interval inside the tile (integer divisions,
//                     the cell coordinates being monotone in r) is counted with LDS atomics; the tile, border included, written once
//   k_hc_centres      one thread per cell; centres appended as 64-bit keys (~votes << 32 | offset)
//   vpk_hough_sort_keys  the key sort of the Hough lines
//   k_hc_radius       one block per centre: distance histogram in LDS (VP_OPT_HOUGH_CIRCLES_LDS 0, or too many bins: a slice of a
//                     context-owned device buffer per block, sized by the centre count), the group walk in one wave with ballots over the
//                     empty bins
//   k_hc_rank         cmpAccum rank of every supported circle among the others (a total order: ranks are distinct)
//   k_hc_overlap      one block: the greedy minDist pass, sequential over candidates, parallel over the kept ones; count + triplets
#include "vp_internal.h"
#include <algorithm>
#include <cmath>
#include <cstring>

#define HC_TW 128              // vote tile: bordered accumulator columns
#define HC_TH 64               // and rows (32 KiB of int counts)
#define HC_NBPDR 10            // bins per dp of radius
#define HC_LDS_MAX (160 << 10)
#define HC_GHIST_BYTES ((size_t)256 << 20)   // budget of the global-histogram form (blocks beyond it loop over more centres)
#define HC_MAX_PARAM 1e9       // param1 / param2 above this: VP_ERR_UNSUPPORTED
#define HC_MAX_R (1 << 20)     // radii above this would overflow OpenCV's int32 ray arithmetic

struct hc_ray {
    int x0, y0, sx, sy;
};

__device__ __forceinline__ int hc_floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }   // b > 0
__device__ __forceinline__ int hc_ceil_div(int a, int b) { return -hc_floor_div(-a, b); }

// narrows [lo, hi] to the r with A <= c0 + r * s <= B
__device__ __forceinline__ void hc_span(int c0, int s, int A, int B, int& lo, int& hi)
{
    if (s > 0) {
        lo = max(lo, hc_ceil_div(A - c0, s));
        hi = min(hi, hc_floor_div(B - c0, s));
    } else if (s < 0) {
        lo = max(lo, hc_ceil_div(c0 - B, -s));
        hi = min(hi, hc_floor_div(c0 - A, -s));
    } else if (c0 < A || c0 > B) {
        hi = lo - 1;
    }
}

// grid ceil(w * h / 4096), 256 threads of 16 pixels each.  rend[2p + k]: the last r of sign k's run (OpenCV's loop from minR until the
// first cell outside the accumulator), minR - 1 when the cell at minR is already outside.  The cells along a ray are monotone in r, so
// the inside r form one interval and the run is its part from minR on.
__global__ __launch_bounds__(256) void k_hc_points(const uint8_t* __restrict__ edges, const short2* __restrict__ grad, int w, int h, float idp,
                                                   int acols, int arows, int min_r, int max_r, hc_ray* __restrict__ rays, int* __restrict__ rend,
                                                   u32* __restrict__ pxy, u32* __restrict__ npts)
{
    __shared__ u32 wsum[4], wbase[4];
    const size_t npx = (size_t)w * h;
    const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 16;
    u32 bits = 0;
    for (int k = 0; k < 16; k++) {
        const size_t i = i0 + k;
        if (i < npx && edges[i]) {
            const short2 g = grad[i];
            if (g.x != 0 || g.y != 0) bits |= 1u << k;     // |g| >= 1 for every non-zero integer gradient
        }
    }
    const u32 cnt = __popc(bits);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 v = cnt;
    for (int d = 1; d < 64; d <<= 1) {
        const u32 t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const u32 tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        u32 b = tot ? atomicAdd(npts, tot) : 0;
        for (int q = 0; q < 4; q++) { wbase[q] = b; b += wsum[q]; }
    }
    __syncthreads();
    u32 o = wbase[wave] + v - cnt;
    const int AX = (acols << 10) - 1, AY = (arows << 10) - 1;
    while (bits) {
        const int k = __ffs(bits) - 1;
        bits &= bits - 1;
        const size_t i = i0 + k;
        const u32 y = (u32)(i / (unsigned)w), x = (u32)(i - (size_t)y * w);
        const short2 g = grad[i];
        const float vx = (float)g.x, vy = (float)g.y;
        const float mag = __fsqrt_rn(__fadd_rn(__fmul_rn(vx, vx), __fmul_rn(vy, vy)));
        hc_ray r;
        r.sx = __float2int_rn(__fdiv_rn(__fmul_rn(__fmul_rn(vx, idp), 1024.f), mag));
        r.sy = __float2int_rn(__fdiv_rn(__fmul_rn(__fmul_rn(vy, idp), 1024.f), mag));
        r.x0 = __float2int_rn(__fmul_rn(__fmul_rn((float)x, idp), 1024.f));
        r.y0 = __float2int_rn(__fmul_rn(__fmul_rn((float)y, idp), 1024.f));
        rays[o] = r;
        for (int s = 0; s < 2; s++) {
            const int sx = s ? -r.sx : r.sx, sy = s ? -r.sy : r.sy;
            int lo = min_r, hi = max_r;
            hc_span(r.x0, sx, 0, AX, lo, hi);
            hc_span(r.y0, sy, 0, AY, lo, hi);
            rend[2 * o + s] = (lo == min_r && hi >= lo) ? hi : min_r - 1;
        }
        pxy[o] = x | (y << 16);
        o++;
    }
}

// grid (tiles across, tiles down), 256 threads; tile (tx, ty) holds bordered cells [ty * HC_TH, +HC_TH) x [tx * HC_TW, +HC_TW)
__global__ __launch_bounds__(256) void k_hc_vote(const hc_ray* __restrict__ rays, const int* __restrict__ rend, const u32* __restrict__ npts_p,
                                                 int acols, int arows, int min_r, int* __restrict__ acc)
{
    __shared__ int tile[HC_TH * HC_TW];
    for (int i = threadIdx.x; i < HC_TH * HC_TW; i += 256) tile[i] = 0;
    __syncthreads();
    const int bx0 = blockIdx.x * HC_TW - 1, by0 = blockIdx.y * HC_TH - 1;   // unbordered cell range of the tile
    const int bx1 = bx0 + HC_TW - 1, by1 = by0 + HC_TH - 1;
    const u32 nr = 2 * *npts_p;
    for (u32 q = threadIdx.x; q < nr; q += 256) {
        const int e = rend[q];
        if (e < min_r) continue;
        const hc_ray r = rays[q >> 1];
        const int sx = (q & 1) ? -r.sx : r.sx, sy = (q & 1) ? -r.sy : r.sy;
        const int xa = (r.x0 + min_r * sx) >> 10, xb = (r.x0 + e * sx) >> 10;
        const int ya = (r.y0 + min_r * sy) >> 10, yb = (r.y0 + e * sy) >> 10;
        if (max(xa, xb) < bx0 || min(xa, xb) > bx1 || max(ya, yb) < by0 || min(ya, yb) > by1) continue;
        int lo = min_r, hi = e;
        hc_span(r.x0, sx, bx0 << 10, (bx1 << 10) + 1023, lo, hi);
        hc_span(r.y0, sy, by0 << 10, (by1 << 10) + 1023, lo, hi);
        int x1 = r.x0 + lo * sx, y1 = r.y0 + lo * sy;
        for (int k = lo; k <= hi; k++, x1 += sx, y1 += sy)
            atomicAdd(&tile[((y1 >> 10) - by0) * HC_TW + ((x1 >> 10) - bx0)], 1);
    }
    __syncthreads();
    const int stride = acols + 2;
    for (int i = threadIdx.x; i < HC_TH * HC_TW; i += 256) {
        const int Y = by0 + 1 + i / HC_TW, X = bx0 + 1 + i % HC_TW;
        if (X < stride && Y < arows + 2) acc[(size_t)Y * stride + X] = tile[i];
    }
}

// grid ceil(arows * acols / 256)
__global__ __launch_bounds__(256) void k_hc_centres(const int* __restrict__ acc, int acols, int arows, int thresh, u64* __restrict__ keys,
                                                    size_t kcap, u32* __restrict__ nkeys)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool pk = false;
    u64 key = 0;
    if (i < (size_t)arows * acols) {
        const int y = (int)(i / (unsigned)acols) + 1, x = (int)(i - (size_t)(y - 1) * acols) + 1;
        const int stride = acols + 2;
        const size_t base = (size_t)y * stride + x;
        const int v = acc[base];
        pk = v > thresh && v > acc[base - 1] && v >= acc[base + 1] && v > acc[base - stride] && v >= acc[base + stride];
        key = ((u64)(~(u32)v) << 32) | (u32)base;
    }
    const u64 m = __ballot(pk);
    if (m == 0) return;
    const int lane = __lane_id();
    const int leader = __ffsll((long long)m) - 1;
    u32 b = 0;
    if (lane == leader) b = atomicAdd(nkeys, (u32)__popcll(m));
    b = __shfl(b, leader);
    const size_t pos = (size_t)b + __popcll(m & ((1ull << lane) - 1ull));
    if (pk && pos < kcap) keys[pos] = key;
}

// grid min(centres, G), 256 threads; a block takes centres blockIdx.x, + gridDim.x, ...  cand: (cx, cy, r, support bits), appended
template <bool LDS>
__global__ __launch_bounds__(256) void k_hc_radius(const u64* __restrict__ keys, const u32* __restrict__ cnt, const u32* __restrict__ pxy,
                                                   int stride, float dp, int min_r, float min_r2, float max_r2, int nbins, int thresh,
                                                   int* __restrict__ ghist, float4* __restrict__ cand, u32* __restrict__ ncand)
{
    extern __shared__ int hc_bins[];
    int* bins = LDS ? hc_bins : ghist + (size_t)blockIdx.x * nbins;
    const u32 npts = cnt[0], ncent = cnt[1];
    const float fmin_r = (float)min_r;
    for (u32 c = blockIdx.x; c < ncent; c += gridDim.x) {
        for (int i = threadIdx.x; i < nbins; i += 256) bins[i] = 0;
        __syncthreads();
        const u32 ofs = (u32)keys[c];
        const int y = (int)(ofs / (u32)stride), x = (int)(ofs - (u32)y * stride);
        const float cx = __fmul_rn(__fadd_rn((float)x, 0.5f), dp), cy = __fmul_rn(__fadd_rn((float)y, 0.5f), dp);
        for (u32 p = threadIdx.x; p < npts; p += 256) {
            const u32 q = pxy[p];
            const float dx = __fsub_rn(cx, (float)(q & 0xffffu)), dy = __fsub_rn(cy, (float)(q >> 16));
            const float r2 = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
            if (min_r2 <= r2 && r2 <= max_r2) {
                const float d = __fsqrt_rn(r2);
                const int b = __float2int_rn(__fmul_rn(__fdiv_rn(__fsub_rn(d, fmin_r), dp), (float)HC_NBPDR));
                atomicAdd(&bins[max(0, min(nbins - 1, b))], 1);
            }
        }
        __syncthreads();
        if (threadIdx.x < 64) {                     // the walk: one wave, uniform control flow
            const int lane = threadIdx.x;
            int j = nbins - 1, max_count = 0;
            float r_best = 0.f;
            while (j > 0) {
                int up = -1;
                for (; j > 0; j -= 64) {            // highest non-empty bin in [1, j]
                    const int b = j - lane;
                    const u64 m = __ballot(b >= 1 && bins[b] != 0);
                    if (m) { up = j - (__ffsll((long long)m) - 1); break; }
                }
                if (up < 0) break;
                int v = (lane < HC_NBPDR && up - lane >= 0) ? bins[up - lane] : 0;
                for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
                j = max(up - HC_NBPDR, -1);         // where the group's inner loop leaves j
                const float r_cur = __fadd_rn(__fmul_rn(__fdiv_rn(__fdiv_rn((float)(up + j), 2.f), (float)HC_NBPDR), dp), fmin_r);
                if (__fmul_rn((float)v, r_best) >= __fmul_rn((float)max_count, r_cur) || (r_best < 1.1920928955078125e-7f && v >= max_count)) {
                    r_best = r_cur;
                    max_count = v;
                }
                j--;                                // the outer loop's decrement
            }
            if (lane == 0 && max_count > thresh) {
                const u32 k = atomicAdd(ncand, 1u);
                cand[k] = make_float4(cx, cy, r_best, __int_as_float(max_count));
            }
        }
        __syncthreads();
    }
}

__device__ __forceinline__ bool hc_before(const float4& a, const float4& b)   // cmpAccum
{
    const int sa = __float_as_int(a.w), sb = __float_as_int(b.w);
    if (sa != sb) return sa > sb;
    if (a.z != b.z) return a.z > b.z;
    if (a.x != b.x) return a.x < b.x;
    return a.y < b.y;
}

// grid ceil(bound / 256): candidate i goes to its rank among all candidates
__global__ __launch_bounds__(256) void k_hc_rank(const float4* __restrict__ cand, const u32* __restrict__ ncand, float4* __restrict__ sorted)
{
    __shared__ float4 t[256];
    const u32 n = *ncand;
    if (blockIdx.x * 256 >= n) return;
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    const float4 me = i < n ? cand[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    u32 rank = 0;
    for (u32 t0 = 0; t0 < n; t0 += 256) {
        __syncthreads();
        if (t0 + threadIdx.x < n) t[threadIdx.x] = cand[t0 + threadIdx.x];
        __syncthreads();
        const u32 m = min(256u, n - t0);
        for (u32 k = 0; k < m; k++) rank += hc_before(t[k], me);
    }
    if (i < n) sorted[rank] = me;
}

// one block of 1024: out[0] = kept count (u32), then (x, y, r) triplets; kept: their centres
__global__ __launch_bounds__(1024) void k_hc_overlap(const float4* __restrict__ sorted, const u32* __restrict__ ncand, float min_dist2,
                                                     float2* __restrict__ kept, float* __restrict__ out, u32 max_out)
{
    const u32 n = *ncand;
    u32 nk = 0;
    for (u32 i = 0; i < n; i++) {
        const float4 c = sorted[i];
        bool close = false;
        for (u32 k = threadIdx.x; k < nk; k += 1024) {
            const float2 p = kept[k];
            const float dx = __fsub_rn(c.x, p.x), dy = __fsub_rn(c.y, p.y);
            close |= __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)) < min_dist2;
        }
        if (__syncthreads_or(close)) continue;
        if (threadIdx.x == 0) {
            kept[nk] = make_float2(c.x, c.y);
            if (nk < max_out) {
                out[1 + 3 * nk] = c.x;
                out[2 + 3 * nk] = c.y;
                out[3 + 3 * nk] = c.z;
            }
        }
        nk++;
        __syncthreads();
    }
    if (threadIdx.x == 0) ((u32*)out)[0] = nk;
}

int vp_hough_circles_run(vp_ctx* ctx, const uint8_t* d_src, const uint8_t* h_src, size_t stride, int w, int h, double dp, double min_dist,
                         double param1, double param2, int min_radius, int max_radius, float* circles, int max_circles, int* n_circles)
{
    if ((!d_src && !h_src) || !n_circles || w <= 0 || h <= 0 || w > 65535 || h > 65535 || max_circles < 0 || (max_circles > 0 && !circles) ||
        (d_src && stride < (size_t)w))
        return vp_fail(ctx, VP_ERR_INVALID, "hough circles arguments");
    if (!(dp > 0) || !(min_dist > 0) || !(param1 > 0) || !(param2 > 0))
        return vp_fail(ctx, VP_ERR_INVALID, "hough circles: dp, min_dist, param1 and param2 must be positive");
    if (!std::isfinite(dp)) return vp_fail(ctx, VP_ERR_INVALID, "hough circles: dp must be finite");
    if (!(param1 <= HC_MAX_PARAM) || !(param2 <= HC_MAX_PARAM))        // cvRound to int: OpenCV's own arithmetic overflows far above this
        return vp_fail(ctx, VP_ERR_UNSUPPORTED, "hough circles: param1 / param2 above 1e9 are outside the supported range");
    if ((size_t)w * h > ((size_t)1 << 28)) return vp_fail(ctx, VP_ERR_UNSUPPORTED, "hough circles: image above 2^28 pixels");
    if (max_radius < 0) return vp_fail(ctx, VP_ERR_UNSUPPORTED, "hough circles: the centres-only mode (max_radius < 0)");
    // HoughCircles: cvRound of the thresholds, the radius defaults
    const int canny_thresh = (int)std::nearbyint(param1), acc_thresh = (int)std::nearbyint(param2);
    min_radius = std::max(0, min_radius);
    if (max_radius == 0) max_radius = std::max(w, h);
    else if (max_radius <= min_radius) max_radius = min_radius + 2;
    if (min_radius > HC_MAX_R || max_radius > HC_MAX_R) return vp_fail(ctx, VP_ERR_UNSUPPORTED, "hough circles: radius above 2^20");
    const float fdp = std::max((float)dp, 1.f), idp = 1.f / fdp;
    const float fmd = (float)min_dist;
    const float md2 = fmd * fmd;
    const int acols = (int)std::ceil((float)w * idp), arows = (int)std::ceil((float)h * idp);
    const int stride_a = acols + 2;
    const size_t acells = (size_t)(arows + 2) * stride_a;
    const size_t npx = (size_t)w * h;
    const int nbins = (int)std::nearbyint((float)(max_radius - min_radius) / fdp * (float)HC_NBPDR);
    const float min_r2 = (float)min_radius * (float)min_radius, max_r2 = (float)max_radius * (float)max_radius;
    // two neighbours of a row cannot both be centres
    const size_t kcap = std::max<size_t>(1, (size_t)arows * (size_t)((acols + 1) / 2));
    const bool lds = ctx->opt.v[VP_OPT_HOUGH_CIRCLES_LDS] && (size_t)nbins * 4 <= HC_LDS_MAX;
    const size_t ocap = std::min(kcap, (size_t)max_circles);
    const bool packed = h_src || stride == (size_t)w;
    vp_ws_frame W;
    uint8_t *d_img = nullptr, *d_edges;
    vp_canny_ws cw;
    hc_ray* d_rays;
    int *d_rend, *d_acc;
    u32 *d_pxy, *d_cnt;
    u64 *d_k0, *d_k1;
    float4 *d_cand, *d_sorted;
    float2* d_kept;
    float* d_out;
    if (!packed || h_src) W.want(&d_img, npx);
    W.want(&d_edges, npx);
    vp_canny_want(W, w, h, &cw);
    W.want(&d_rays, npx * sizeof(hc_ray));
    W.want(&d_rend, npx * 8);
    W.want(&d_pxy, npx * 4);
    W.want(&d_acc, acells * 4);
    W.want(&d_k0, kcap * 8);
    W.want(&d_k1, kcap * 8);
    W.want(&d_cnt, 16);                      // points, centres, supported circles
    W.want(&d_cand, kcap * 16);
    W.want(&d_sorted, kcap * 16);
    W.want(&d_kept, kcap * 8);
    W.want(&d_out, 4 + ocap * 12);
    int rc = vp_ws_commit(ctx, W, "hough circles workspace");
    if (rc != VP_OK) return rc;
    const uint8_t* src = d_src;
    if (d_img) {
        if (h_src) VP_HIP(ctx, hipMemcpyAsync(d_img, h_src, npx, hipMemcpyHostToDevice, ctx->stream));
        else VP_HIP(ctx, hipMemcpy2DAsync(d_img, (size_t)w, d_src, stride, (size_t)w, h, hipMemcpyDeviceToDevice, ctx->stream));
        src = d_img;
    }
    int lo_t = std::max(1, canny_thresh / 2), hi_t = canny_thresh;
    if (lo_t > hi_t) std::swap(lo_t, hi_t);                      // Canny orders its thresholds (param1 < 1.5)
    rc = vpk_canny_u8(ctx, src, w, h, 1, lo_t, hi_t, d_edges, cw);
    if (rc != VP_OK) return rc;
    const short2* d_grad = cw.grad;
    hipStream_t s = ctx->stream;
    VP_HIP(ctx, hipMemsetAsync(d_cnt, 0, 16, s));
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_hc_points, dim3((unsigned)((npx + 4095) / 4096)), dim3(256), 0, s, d_edges, d_grad, w, h, idp, acols, arows,
                           min_radius, max_radius, d_rays, d_rend, d_pxy, d_cnt);
    }
    VP_HIP(ctx, hipGetLastError());
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_hc_vote, dim3((unsigned)((stride_a + HC_TW - 1) / HC_TW), (unsigned)((arows + 2 + HC_TH - 1) / HC_TH)), dim3(256), 0,
                           s, d_rays, d_rend, d_cnt, acols, arows, min_radius, d_acc);
    }
    VP_HIP(ctx, hipGetLastError());
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_hc_centres, dim3((unsigned)(((size_t)arows * acols + 255) / 256)), dim3(256), 0, s, d_acc, acols, arows, acc_thresh,
                           d_k0, kcap, d_cnt + 1);
    }
    VP_HIP(ctx, hipGetLastError());
    u32* hs = (u32*)vp_hstage(ctx, 16);
    if (!hs) return vp_fail(ctx, VP_ERR_NOMEM, "pinned staging");
    VP_HIP(ctx, hipMemcpyAsync(hs, d_cnt, 8, hipMemcpyDeviceToHost, s));
    VP_HIP(ctx, hipStreamSynchronize(s));
    const u32 npts = hs[0], ncent = hs[1];
    *n_circles = 0;
    if (npts == 0 || ncent == 0 || nbins <= 0) return VP_OK;     // no point, no centre, or no bin: cv2 returns nothing
    if ((size_t)ncent > kcap) return vp_fail(ctx, VP_ERR_HIP, "hough circles: centre count above its bound");
    // the global-histogram form: one slice of nbins counters per block, sized now that the centres are counted (a context-owned
    // buffer that only grows: the workspace's carve of this call is in use)
    size_t ghist_blocks = 0;
    if (!lds) {
        ghist_blocks = std::max<size_t>(1, std::min<size_t>({(size_t)ncent, 1024, HC_GHIST_BYTES / ((size_t)nbins * 4)}));
        const size_t gbytes = ghist_blocks * (size_t)nbins * 4;
        if (gbytes > ctx->hc.hist_bytes) {
            if (ctx->hc.hist) { VP_HIP(ctx, hipFree(ctx->hc.hist)); ctx->hc.hist = nullptr; ctx->hc.hist_bytes = 0; }   // stream idle: synchronised above
            VP_HIP(ctx, hipMalloc(&ctx->hc.hist, gbytes));
            ctx->hc.hist_bytes = gbytes;
        }
    }
    int* d_ghist = (int*)ctx->hc.hist;
    u64* d_keys = nullptr;
    rc = vpk_hough_sort_keys(ctx, d_k0, d_k1, kcap, d_cnt + 1, 1, ncent, &d_keys);
    if (rc != VP_OK) return rc;
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        if (lds) {
            const size_t lbytes = (size_t)nbins * 4;
            if (lbytes > (64 << 10))
                VP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_hc_radius<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                (int)lbytes));
            hipLaunchKernelGGL(k_hc_radius<true>, dim3(ncent), dim3(256), lbytes, s, d_keys, d_cnt, d_pxy, stride_a, fdp, min_radius, min_r2,
                               max_r2, nbins, acc_thresh, (int*)nullptr, d_cand, d_cnt + 2);
        } else {
            hipLaunchKernelGGL(k_hc_radius<false>, dim3((unsigned)std::min<size_t>(ncent, ghist_blocks)), dim3(256), 0, s, d_keys, d_cnt, d_pxy,
                               stride_a, fdp, min_radius, min_r2, max_r2, nbins, acc_thresh, d_ghist, d_cand, d_cnt + 2);
        }
    }
    VP_HIP(ctx, hipGetLastError());
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_hc_rank, dim3((ncent + 255) / 256), dim3(256), 0, s, d_cand, d_cnt + 2, d_sorted);
        hipLaunchKernelGGL(k_hc_overlap, dim3(1), dim3(1024), 0, s, d_sorted, d_cnt + 2, md2, d_kept, d_out, (u32)ocap);
    }
    VP_HIP(ctx, hipGetLastError());
    const size_t nout = std::min((size_t)ncent, ocap);
    float* hl = (float*)vp_hstage(ctx, 4 + nout * 12);
    if (!hl) return vp_fail(ctx, VP_ERR_NOMEM, "pinned staging");
    VP_HIP(ctx, hipMemcpyAsync(hl, d_out, 4 + nout * 12, hipMemcpyDeviceToHost, s));
    VP_HIP(ctx, hipStreamSynchronize(s));
    u32 kept;
    memcpy(&kept, hl, 4);
    if (kept > ncent) return vp_fail(ctx, VP_ERR_HIP, "hough circles: circle count above its bound");
    *n_circles = (int)kept;
    if (circles && max_circles > 0) memcpy(circles, hl + 1, std::min((size_t)kept, (size_t)max_circles) * 12);
    return VP_OK;
}

void vp_hough_circles_teardown(vp_ctx* ctx)
{
    if (ctx->hc.hist) (void)hipFree(ctx->hc.hist);
    ctx->hc = vp_hough_circles_state{};
}
