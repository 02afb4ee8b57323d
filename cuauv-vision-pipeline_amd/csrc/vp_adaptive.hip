// cv2.adaptiveThreshold(src, maxValue, ADAPTIVE_THRESH_GAUSSIAN_C, type, blockSize, C) on 8-bit images (utils/color.py:257-292
// adaptive_threshold_gaussian / adaptive_threshold_gaussian_inv).
//
// OpenCV 4.x (imgproc/src/thresh.cpp) blurs a float32 copy of the image with GaussianBlur(blockSize x blockSize, sigma 0,
// BORDER_REPLICATE | BORDER_ISOLATED), converts the blur back to 8 bits (round half to even) and compares as the mean method does.
// Its float32 sums depend on the build, so the contract here is the exact Gaussian-weighted mean of OpenCV's own float32 taps
// (getGaussianKernel(blockSize, 0, CV_32F), separable, replicated borders), rounded half to even.
//
// Every float32 tap is an integer t_i times 2^-E, E the smallest exponent that makes them all integers (E <= 39, t_i < 2^32 for
// every odd block size up to 511).  The horizontal pass writes the exact row sums H = sum t_i p as u64 (< 255 * 2^40); the vertical
// pass splits each pair sum S = H_a + H_b at bit 24 and accumulates A = sum t_j (S mod 2^24), B = sum t_j (S >> 24) in u64 (the host
// checks that neither can overflow), so that V = A + B 2^24 is the exact 2-D sum; the mean V / 2^(E_h + E_v) is rounded half to even
// in 128 bits.  No floating point runs in the kernels.
#include "vp_internal.h"
#include <cmath>
#include <cstring>

#define AG_TILE 1024          // outputs per block of the horizontal pass
#define AG_HALF (VP_AGAUSS_MAX_BLOCK / 2 + 1)

// grid (ceil(w / AG_TILE), h, frames), 256 threads: the block's piece of the row (+ halo, replicated) in LDS; taps[0..r], taps[r] the centre
__global__ __launch_bounds__(256) void k_agauss_h(const uint8_t* __restrict__ src, size_t stride, size_t fstride, int w, int h,
                                                  const u32* __restrict__ taps, int r, uint64_t* __restrict__ tmp)
{
    extern __shared__ uint8_t ag_lds[];
    __shared__ u32 tp[AG_HALF];
    const int y = blockIdx.y, f = blockIdx.z, x0 = blockIdx.x * AG_TILE;
    const int nx = min(AG_TILE, w - x0);
    const uint8_t* row = src + (size_t)f * fstride + (size_t)y * stride;
    for (int i = threadIdx.x; i <= r; i += 256) tp[i] = taps[i];
    for (int i = threadIdx.x; i < nx + 2 * r; i += 256) ag_lds[i] = row[min(max(x0 - r + i, 0), w - 1)];
    __syncthreads();
    uint64_t* out = tmp + ((size_t)f * h + y) * w + x0;
    for (int o = threadIdx.x; o < nx; o += 256) {
        const uint8_t* p = ag_lds + o;               // tap 0 at pixel x - r
        uint64_t s = (uint64_t)tp[r] * p[r];
        for (int k = 0; k < r; k++) s += (uint64_t)tp[k] * (u32)(p[k] + p[2 * r - k]);
        out[o] = s;
    }
}

// grid (ceil(w / 256), h, frames), 256 threads: thread = one output pixel; rounding, the compare and the imax / 0 write fused
__global__ __launch_bounds__(256) void k_agauss_v(const uint8_t* __restrict__ src, size_t stride, size_t fstride, const uint64_t* __restrict__ tmp,
                                                  int w, int h, const u32* __restrict__ taps, int r, int shift, int imax, int idelta, int inv,
                                                  uint8_t* __restrict__ dst)
{
    __shared__ u32 tp[AG_HALF];
    for (int i = threadIdx.x; i <= r; i += 256) tp[i] = taps[i];
    __syncthreads();
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, f = blockIdx.z;
    if (x >= w) return;
    const uint64_t* col = tmp + (size_t)f * h * w + x;
    const uint64_t lo24 = (1ull << 24) - 1;
    const uint64_t hc = col[(size_t)y * w];
    uint64_t a = (uint64_t)tp[r] * (u32)(hc & lo24), b = (uint64_t)tp[r] * (u32)(hc >> 24);
    if (y - r >= 0 && y + r < h) {
        const uint64_t* p = col + (size_t)(y - r) * w;
        for (int k = 0; k < r; k++) {
            const uint64_t s = p[(size_t)k * w] + p[(size_t)(2 * r - k) * w];
            a += (uint64_t)tp[k] * (u32)(s & lo24);
            b += (uint64_t)tp[k] * (u32)(s >> 24);
        }
    } else {
        for (int k = 0; k < r; k++) {
            const uint64_t s = col[(size_t)max(y - r + k, 0) * w] + col[(size_t)min(y + r - k, h - 1) * w];
            a += (uint64_t)tp[k] * (u32)(s & lo24);
            b += (uint64_t)tp[k] * (u32)(s >> 24);
        }
    }
    const unsigned __int128 v = (unsigned __int128)a + ((unsigned __int128)b << 24);
    unsigned __int128 q = v >> shift;
    if (shift > 0) {
        const unsigned __int128 rem = v - (q << shift), half = (unsigned __int128)1 << (shift - 1);
        if (rem > half || (rem == half && (q & 1))) q += 1;
    }
    const int mean = q > 255 ? 255 : (int)q;
    const int diff = (int)src[(size_t)f * fstride + (size_t)y * stride + x] - mean;
    const bool on = inv ? diff <= -idelta : diff > -idelta;
    dst[((size_t)f * h + y) * w + x] = (uint8_t)(on ? imax : 0);
}

// float32 taps of getGaussianKernel(n, 0, CV_32F) (n = 1: the single tap 1.0) as integers t[0..n/2] (t[n/2] the centre) times 2^-e
static int agauss_int_taps(int n, u32* t, int* e_out)
{
    float fk[AG_HALF];
    const int r = n / 2;
    if (n == 1) {
        fk[0] = 1.0f;
    } else {
        double k[VP_AGAUSS_MAX_BLOCK + 1];
        vp_gaussian_kernel_f64(n, 0, k);
        for (int i = 0; i <= r; i++) fk[i] = (float)k[i];
    }
    int e = 0;
    for (int i = 0; i <= r; i++) {
        if (!(fk[i] > 0)) return VP_ERR_UNSUPPORTED;
        int ex = 0;
        uint32_t m = (uint32_t)std::ldexp((double)std::frexp(fk[i], &ex), 24);   // fk = m * 2^(ex - 24)
        int q = ex - 24;
        while (!(m & 1)) { m >>= 1; q++; }
        e = std::max(e, -q);
    }
    for (int i = 0; i <= r; i++) {
        const double v = std::ldexp((double)fk[i], e);
        if (v >= 4294967296.0) return VP_ERR_UNSUPPORTED;
        t[i] = (u32)v;
    }
    *e_out = e;
    return VP_OK;
}

// the context's device copy of block size n's integer taps (made on first use, 8 slots replaced in turn).  *slot receives the slot
// used; slot `keep` (one the same call still needs, or -1) is never the one replaced.
static int agauss_slot(vp_ctx* ctx, int n, int keep, int* slot, const u32** d_taps, u32* h_taps, int* e)
{
    if (!ctx->agauss.taps) {
        void* p = nullptr;
        VP_HIP(ctx, hipMalloc(&p, 8 * AG_HALF * sizeof(u32)));
        ctx->agauss.taps = (u32*)p;
    }
    for (int s = 0; s < 8; s++)
        if (ctx->agauss.n[s] == n) {
            *d_taps = ctx->agauss.taps + s * AG_HALF;
            *e = ctx->agauss.e[s];
            memcpy(h_taps, ctx->agauss.host[s], (n / 2 + 1) * sizeof(u32));
            *slot = s;
            return VP_OK;
        }
    if (agauss_int_taps(n, h_taps, e) != VP_OK) return vp_fail(ctx, VP_ERR_UNSUPPORTED, "adaptive threshold: taps outside the integer form");
    int s = ctx->agauss.next;
    if (s == keep) s = (s + 1) & 7;
    ctx->agauss.next = (s + 1) & 7;
    VP_HIP(ctx, hipStreamSynchronize(ctx->stream));      // work queued earlier may still read the slot
    ctx->agauss.n[s] = 0;
    VP_HIP(ctx, hipMemcpy(ctx->agauss.taps + s * AG_HALF, h_taps, (n / 2 + 1) * sizeof(u32), hipMemcpyHostToDevice));
    memcpy(ctx->agauss.host[s], h_taps, (n / 2 + 1) * sizeof(u32));
    ctx->agauss.n[s] = n;
    ctx->agauss.e[s] = *e;
    *d_taps = ctx->agauss.taps + s * AG_HALF;
    *slot = s;
    return VP_OK;
}

void vp_adaptive_teardown(vp_ctx* ctx)
{
    if (ctx->agauss.taps) (void)hipFree(ctx->agauss.taps);
    ctx->agauss.taps = nullptr;
    for (int& n : ctx->agauss.n) n = 0;     // no slot holds taps any more
}

size_t vp_agauss_tmp_bytes(int w, int h, int n) { return (size_t)w * h * n * 8; }

int vpk_adaptive_threshold_gaussian(vp_ctx* ctx, const uint8_t* d_src, size_t stride, size_t fstride, int n, int w, int h, int imax, int idelta,
                                    int inv, int block, uint64_t* d_tmp, uint8_t* d_dst)
{
    // BORDER_ISOLATED: a kernel dimension longer than a one-pixel image side becomes the single tap 1.0 (smooth.dispatch.cpp GaussianBlur)
    const int nh = w == 1 ? 1 : block, nv = h == 1 ? 1 : block;
    u32 th[AG_HALF], tv[AG_HALF];
    const u32 *dh = nullptr, *dv = nullptr;
    int eh = 0, ev = 0, sh_slot = -1, sv_slot = -1;
    int rc = agauss_slot(ctx, nh, -1, &sh_slot, &dh, th, &eh);
    if (rc == VP_OK) rc = agauss_slot(ctx, nv, sh_slot, &sv_slot, &dv, tv, &ev);   // must not evict the horizontal taps
    if (rc == VP_OK && nh != nv && sh_slot == sv_slot) rc = vp_fail(ctx, VP_ERR_INVALID, "adaptive threshold: tap slot reused");
    if (rc != VP_OK) return rc;
    // overflow bounds at p = 255 everywhere: H < 2^63, S = 2 H, S >> 24 < 2^32, A = sum t (S mod 2^24) and B = sum t (S >> 24) < 2^64
    const int rh = nh / 2, rv = nv / 2;
    unsigned __int128 sh = th[rh], sv = 0;
    for (int i = 0; i < rh; i++) sh += 2 * (unsigned __int128)th[i];
    for (int i = 0; i <= rv; i++) sv += tv[i];
    const unsigned __int128 smax = 2 * 255 * sh, lim = (unsigned __int128)1 << 64;
    if (smax >= lim || (smax >> 24) >= ((unsigned __int128)1 << 32) || ((unsigned __int128)((1u << 24) - 1)) * sv >= lim || (smax >> 24) * sv >= lim)
        return vp_fail(ctx, VP_ERR_UNSUPPORTED, "adaptive threshold: integer sums would overflow");
    vp_prof_scope ps(ctx, VPK_OTHER);
    hipLaunchKernelGGL(k_agauss_h, dim3((unsigned)((w + AG_TILE - 1) / AG_TILE), (unsigned)h, (unsigned)n), dim3(256), (size_t)AG_TILE + 2 * rh + 16,
                       ctx->stream, d_src, stride, fstride, w, h, dh, rh, d_tmp);
    hipLaunchKernelGGL(k_agauss_v, dim3((unsigned)((w + 255) / 256), (unsigned)h, (unsigned)n), dim3(256), 0, ctx->stream, d_src, stride, fstride,
                       (const uint64_t*)d_tmp, w, h, dv, rv, eh + ev, imax, idelta, inv, d_dst);
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
