// Stereo block matching (tests/stereo_restate.py is the statement; geometry and LDS layout: vp_stereo_plan.h).
//   k_stereo_prefilter  the capped horizontal Sobel of both images as bytes, and the invalid value into every pixel of the result
//   k_stereo_match      a block owns a strip of candidate columns and marches down a band of rows.  It keeps, per column and disparity,
//                       the vertical sum of absolute differences over the window's rows (add the entering row, drop the leaving one),
//                       two 16-bit sums to a word; a horizontal pass turns them into window sums by a running difference; then the
//                       threads that share a pixel scan their part of the disparities.  The cost volume never leaves LDS.
//   k_stereo_depth      int16 disparity -> float32 metres
#include "vp_internal.h"
#include "vp_stereo_plan.h"

struct sb_args {
    int w, h, nd, min_disp, cap, texture, uniq;
    vp_stereo_plan P;
};

__global__ __launch_bounds__(256) void k_stereo_prefilter(const uint8_t* __restrict__ left, size_t lstride, const uint8_t* __restrict__ right, size_t rstride, int w, int h,
                                                          int cap, uint8_t* __restrict__ out_left, uint8_t* __restrict__ out_right, size_t pitch,
                                                          int16_t* __restrict__ disp, size_t dstride, int16_t inv)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const bool second = blockIdx.z != 0;
    const uint8_t* src = second ? right : left;
    const size_t stride = second ? rstride : lstride;
    int v = cap;
    if (x >= 1 && x <= w - 2) {
        // rows reflected without the edge row; a single row stands for its neighbours
        const int ya = h == 1 ? 0 : (y == 0 ? 1 : y - 1), yb = h == 1 ? 0 : (y == h - 1 ? h - 2 : y + 1);
        const uint8_t *a = src + (size_t)ya * stride + x, *m = src + (size_t)y * stride + x, *b = src + (size_t)yb * stride + x;
        int s = (int)a[1] - (int)a[-1] + 2 * ((int)m[1] - (int)m[-1]) + (int)b[1] - (int)b[-1];
        s = s < -cap ? -cap : (s > cap ? cap : s);
        v = s + cap;
    }
    (second ? out_right : out_left)[(size_t)y * pitch + x] = (uint8_t)v;
    if (!second) disp[(size_t)y * dstride + x] = inv;
}

__device__ __forceinline__ u32 sb_absdiff(int a, int b) { return (u32)(a > b ? a - b : b - a); }

__global__ __launch_bounds__(SB_THREADS) void k_stereo_match(const uint8_t* __restrict__ pl, const uint8_t* __restrict__ pr, sb_args A, int16_t* __restrict__ disp,
                                                             size_t dstride)
{
    extern __shared__ __attribute__((aligned(16))) u32 sb_lds[];
    const vp_stereo_plan& P = A.P;
    const int t = threadIdx.x, r = P.r, nd = A.nd, ndp = P.ndp, ncols = P.ncols, nrcols = P.nrcols, tw = P.strip_cols;
    u32* V = sb_lds + P.off_v;                                     // [ncols][ndp]: vertical sums of disparities 2 dp (low half) and 2 dp + 1
    unsigned short* H = (unsigned short*)(sb_lds + P.off_h);       // [nd][hpitch]: window sums; even disparities first, then the odd ones
    u32* T = sb_lds + P.off_t;                                     // [ncols]: vertical sums of |left - cap|
    uint8_t* lnew = (uint8_t*)(sb_lds + P.off_rows);
    uint8_t* lold = lnew + P.lpitch;
    uint8_t* rnew = lold + P.lpitch;
    uint8_t* rold = rnew + P.rpitch;
    u32* red1 = sb_lds + P.off_red;
    u32* red2 = red1 + SB_THREADS;

    const int xs = P.cx0 + (int)blockIdx.x * tw;                   // the strip's first candidate column
    const int y_first = P.cy0 + (int)blockIdx.y * P.band_rows;
    const int y_end = min(P.cy0 + P.ch, y_first + P.band_rows);    // one past the band's last candidate row
    const int px_end = min(tw, P.cx0 + P.cw - xs);                 // candidate pixels of this strip
    const int colbase = xs - r;                                    // image column of vertical-sum column 0
    const int rbase = colbase - (A.min_disp + nd - 1);             // image column of the staged right row's byte 0
    const size_t pitch = P.pitch;

    for (int i = t; i < ncols * ndp; i += SB_THREADS) V[i] = 0;
    if (t < ncols) T[t] = 0;

    // this thread's items of the vertical pass: (column, disparity pair) = (i / ndp, i % ndp) for i = t, t + 256, ...
    const int c_first = t / ndp, dp_first = t - c_first * ndp, c_step = SB_THREADS / ndp, dp_step = SB_THREADS - c_step * ndp;
    // ... of the horizontal pass: disparity pair hdp, columns [hx0, hx1)
    const int hseg = t / ndp, hdp = t - hseg * ndp;
    const int hx0 = hseg < P.segs ? min(tw, hseg * P.seg_cols) : 0, hx1 = hseg < P.segs ? min(tw, hx0 + P.seg_cols) : 0;
    // ... of the scan: pixel sx, disparities [sd0, sd0 + nd / parts)
    const int part = t / tw, sx = t - part * tw, sdn = nd / P.parts, sd0 = part * sdn;
    const int hp = P.hpitch;

    for (int ya = y_first - r; ya < y_end + r; ya++) {
        const int yo = ya - (2 * r + 1);
        const bool has_old = yo >= y_first - r;
        __syncthreads();                                           // the rows of the step before have been read (and V, T zeroed)
        for (int j = t; j < ncols; j += SB_THREADS) {
            const int col = colbase + j;
            const bool in = col >= 0 && col < A.w;
            lnew[j] = in ? pl[(size_t)ya * pitch + col] : (uint8_t)0;
            lold[j] = in && has_old ? pl[(size_t)yo * pitch + col] : (uint8_t)0;
        }
        for (int j = t; j < nrcols; j += SB_THREADS) {
            const int col = rbase + j;
            const bool in = col >= 0 && col < A.w;
            rnew[j] = in ? pr[(size_t)ya * pitch + col] : (uint8_t)0;
            rold[j] = in && has_old ? pr[(size_t)yo * pitch + col] : (uint8_t)0;
        }
        __syncthreads();
        // vertical pass: add row ya, drop row yo (a band's first 2 r + 1 rows drop nothing: their old bytes are zeros on both sides)
        for (int c = c_first, dp = dp_first; c < ncols;) {
            const int ln = lnew[c], lo = lold[c], j = c + nd - 1 - 2 * dp;      // right byte of the even disparity; the odd one is at j - 1
            const u32 add = sb_absdiff(ln, rnew[j]) | (sb_absdiff(ln, rnew[j - 1]) << 16);
            const u32 sub = sb_absdiff(lo, rold[j]) | (sb_absdiff(lo, rold[j - 1]) << 16);
            V[c * ndp + dp] += add - sub;                                        // no half borrows: each half still holds what it drops
            c += c_step;
            dp += dp_step;
            if (dp >= ndp) { dp -= ndp; c++; }
        }
        if (t < ncols) {
            const bool in = colbase + t >= 0 && colbase + t < A.w;
            if (in) T[t] += sb_absdiff(lnew[t], A.cap) - (has_old ? sb_absdiff(lold[t], A.cap) : 0u);
        }
        if (ya < y_first + r) continue;                            // (uniform) the window's rows are not all in yet
        const int y = ya - r;
        __syncthreads();
        // horizontal pass: window sums of both halves at once, by a running difference along the segment
        if (hx0 < hx1) {
            u32 acc = 0;
            for (int k = 0; k <= 2 * r; k++) acc += V[(hx0 + k) * ndp + hdp];
            for (int x = hx0;; x++) {
                H[hdp * hp + x] = (unsigned short)(acc & 0xffffu);
                H[(ndp + hdp) * hp + x] = (unsigned short)(acc >> 16);
                if (x + 1 == hx1) break;
                acc += V[(x + 2 * r + 1) * ndp + hdp];
                acc -= V[x * ndp + hdp];
            }
        }
        __syncthreads();
        // scan, first half: the smallest cost of this thread's disparities, ties to the larger disparity
        u32 key = 0xffffffffu;
        for (int d = sd0; d < sd0 + sdn; d++) {
            const u32 c = H[((d & 1) * ndp + (d >> 1)) * hp + sx];
            key = min(key, (c << 8) | (u32)(255 - d));
        }
        red1[t] = key;
        __syncthreads();
        key = red1[sx];
        for (int q = 1; q < P.parts; q++) key = min(key, red1[q * tw + sx]);
        const int ds = 255 - (int)(key & 255u), cmin = (int)(key >> 8);
        if (A.uniq > 0) {                                          // (uniform) second half: the best rival more than one disparity away
            u32 rival = 0xffffffffu;
            for (int d = sd0; d < sd0 + sdn; d++) {
                const u32 c = H[((d & 1) * ndp + (d >> 1)) * hp + sx];
                if (d < ds - 1 || d > ds + 1) rival = min(rival, c);
            }
            red2[t] = rival;
            __syncthreads();
        }
        if (part == 0 && sx < px_end) {
            u32 tex = 0;
            for (int k = 0; k <= 2 * r; k++) tex += T[sx + k];
            int16_t out = (int16_t)vp_stereo_invalid(A.min_disp);
            bool keep = (long long)tex >= (long long)A.texture;
            if (keep && A.uniq > 0) {
                u32 rival = red2[sx];
                for (int q = 1; q < P.parts; q++) rival = min(rival, red2[q * tw + sx]);
                keep = !(rival <= (u32)(cmin + cmin * A.uniq / 100));
            }
            if (keep) {
                const int dm = ds > 0 ? ds - 1 : ds + 1, dq = ds < nd - 1 ? ds + 1 : ds - 1;
                const int pm = H[((dm & 1) * ndp + (dm >> 1)) * hp + sx], pp = H[((dq & 1) * ndp + (dq >> 1)) * hp + sx];
                out = vp_stereo_subpixel(cmin, pm, pp, A.min_disp + ds);
            }
            disp[(size_t)y * dstride + xs + sx] = out;
        }
    }
}

__global__ __launch_bounds__(256) void k_stereo_depth(const int16_t* __restrict__ disp, size_t sstride, int w, int h, double fb, float* __restrict__ depth, size_t dstride)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    depth[(size_t)y * dstride + x] = vp_stereo_depth(fb, disp[(size_t)y * sstride + x]);
}

// both prefiltered images (rows of `pitch` bytes) and the invalid value into every pixel of the result: the first launch of the block
// matcher and of semi-global matching (vp_sgm.hip)
int vpk_stereo_prefilter(vp_ctx* ctx, const uint8_t* d_left, size_t lstride, const uint8_t* d_right, size_t rstride, int w, int h, int cap, int min_disp, uint8_t* pl,
                         uint8_t* pr, size_t pitch, int16_t* d_disp, size_t dstride)
{
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_stereo_prefilter, dim3((unsigned)((w + 255) / 256), (unsigned)h, 2), dim3(256), 0, ctx->stream, d_left, lstride, d_right, rstride, w, h, cap, pl,
                           pr, pitch, d_disp, dstride / 2, (int16_t)vp_stereo_invalid(min_disp));
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

int vpk_stereo_bm(vp_ctx* ctx, const uint8_t* d_left, size_t lstride, const uint8_t* d_right, size_t rstride, int w, int h, int nd, int min_disp, int cap, int texture,
                  int uniq, const vp_stereo_plan& P, uint8_t* d_ws, int16_t* d_disp, size_t dstride)
{
    uint8_t *pl = d_ws, *pr = d_ws + P.off_right;
    if (int rc = vpk_stereo_prefilter(ctx, d_left, lstride, d_right, rstride, w, h, cap, min_disp, pl, pr, P.pitch, d_disp, dstride)) return rc;
    if (!P.cw) return VP_OK;
    if (P.lds_bytes > SB_LDS_BYTES) return vp_fail(ctx, VP_ERR_UNSUPPORTED, "stereo: the strip's tables are above the LDS budget");
    sb_args A = {w, h, nd, min_disp, cap, texture, uniq, P};
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_stereo_match, dim3(P.grid_x, P.grid_y), dim3(SB_THREADS), P.lds_bytes, ctx->stream, pl, pr, A, d_disp, dstride / 2);
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

int vpk_stereo_depth(vp_ctx* ctx, const int16_t* d_disp, size_t sstride, int w, int h, double fb, float* d_depth, size_t dstride)
{
    vp_prof_scope ps(ctx, VPK_OTHER);
    hipLaunchKernelGGL(k_stereo_depth, dim3((unsigned)((w + 255) / 256), (unsigned)h), dim3(256), 0, ctx->stream, d_disp, sstride / 2, w, h, fb, d_depth, dstride / 4);
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
