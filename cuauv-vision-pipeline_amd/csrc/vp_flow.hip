// Pyramidal Lucas-Kanade point tracking, cv2.calcOpticalFlowPyrLK, on uint8 single-channel pyramids (the
// statement: tests/flow_restate.py; checks, level rule, reflection and LDS layout: vp_flow_plan.h).  One launch for all levels and
// all points: a workgroup of one wave per point runs the whole coarse-to-fine loop.  Trip counts differ from point to point, never
// inside a workgroup: every value a branch depends on is the same in all 64 lanes (the points, and sums that were added across the
// wave), so every barrier is reached by all lanes or by none.
//
// Per level the (ww + 3) x (wh + 3) patch of the first image round the window is staged in LDS once, through index reflection; the
// Scharr pair is formed from it for the (ww + 1) x (wh + 1) pixels the window's bilinear samples touch (0 outside the level), and
// from both the int16 window I, Ix, Iy with the exact 64-bit sums of Ix Ix, Ix Iy, Iy Iy.  Per iteration each lane gathers its share
// of the second image's window (every index reflected and clamped), keeps 64-bit sums of diff Ix and diff Iy, the wave adds them
// with cross-lane moves, and every lane takes the same step: OpenCV's sequence in double, in the one order the statement writes
// down, rounded to float32 where OpenCV holds a float.  This unit is compiled without floating-point contraction.
#include "vp_internal.h"
#include "vp_flow_plan.h"

struct vp_lk_args {
    int win_w, win_h, levels, max_count, flags;
    unsigned off_deriv, off_win;
    double eps2, min_eig;
};

__device__ __forceinline__ int lk_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// cv2's four fixed-point weights of the fractions a (x) and b (y); cvRound is round-half-even
__device__ __forceinline__ void lk_weights(float a, float b, int& w00, int& w01, int& w10, int& w11)
{
    const float s = (float)(1 << LK_W_BITS);
    w00 = (int)rintf((1.f - a) * (1.f - b) * s);
    w01 = (int)rintf(a * (1.f - b) * s);
    w10 = (int)rintf((1.f - a) * b * s);
    w11 = (1 << LK_W_BITS) - w00 - w01 - w10;
}

// cv2's range test on the floored floats, before any of them becomes an integer (false for anything that is not finite)
__device__ __forceinline__ bool lk_in_range(float fx, float fy, int ww, int wh, int cols, int rows)
{
    return fx >= (float)-ww && fx < (float)cols && fy >= (float)-wh && fy < (float)rows;
}

__device__ __forceinline__ long long lk_wave_sum(long long v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// the window of the second image at (jx, jy) with weights w: sum diff Ix, sum diff Iy (want_abs 0) or sum |diff| in s1 (want_abs 1)
__device__ __forceinline__ void lk_mismatch(const uint8_t* __restrict__ J, size_t stride, int cols, int rows, int jx, int jy, int w00, int w01, int w10, int w11, int ww,
                                            int wh, const int16_t* s_I, const int16_t* s_Ix, const int16_t* s_Iy, int want_abs, long long& s1, long long& s2)
{
    const int area = ww * wh, lane = threadIdx.x;
    const int step_y = LK_LANES / ww, step_x = LK_LANES - step_y * ww;
    int x = lane % ww, y = lane / ww;
    long long a1 = 0, a2 = 0;
    for (int k = lane; k < area; k += LK_LANES) {
        const int x0 = vp_lk_reflect(jx + x, cols), x1 = vp_lk_reflect(jx + x + 1, cols);
        const uint8_t* r0 = J + (size_t)vp_lk_reflect(jy + y, rows) * stride;
        const uint8_t* r1 = J + (size_t)vp_lk_reflect(jy + y + 1, rows) * stride;
        const int diff = lk_descale((int)r0[x0] * w00 + (int)r0[x1] * w01 + (int)r1[x0] * w10 + (int)r1[x1] * w11, LK_W_BITS - 5) - (int)s_I[k];
        if (want_abs) a1 += diff < 0 ? -diff : diff;
        else {
            a1 += diff * (int)s_Ix[k];
            a2 += diff * (int)s_Iy[k];
        }
        x += step_x;
        y += step_y;
        if (x >= ww) { x -= ww; y++; }
    }
    s1 = lk_wave_sum(a1);
    s2 = want_abs ? 0 : lk_wave_sum(a2);
}

// out: four 32-bit words per point - x, y, err as float32 bits, status
__global__ __launch_bounds__(LK_LANES) void k_lk_flow(vp_lk_levels L, vp_lk_args A, const float* __restrict__ pts, const float* __restrict__ guess, u32* __restrict__ out)
{
    extern __shared__ __align__(16) uint8_t lk_lds[];
    const int lane = threadIdx.x, ww = A.win_w, wh = A.win_h, area = ww * wh, pw = ww + 3, dw = ww + 1;
    uint8_t* s_patch = lk_lds;
    short2* s_deriv = reinterpret_cast<short2*>(lk_lds + A.off_deriv);
    int16_t* s_I = reinterpret_cast<int16_t*>(lk_lds + A.off_win);
    int16_t* s_Ix = s_I + area;
    int16_t* s_Iy = s_Ix + area;
    u32* o = out + 4 * (size_t)blockIdx.x;

    const float ptx = pts[2 * (size_t)blockIdx.x], pty = pts[2 * (size_t)blockIdx.x + 1];
    const float gsx = guess ? guess[2 * (size_t)blockIdx.x] : ptx, gsy = guess ? guess[2 * (size_t)blockIdx.x + 1] : pty;
    if (!(fabsf(ptx) <= LK_COORD_LIMIT && fabsf(pty) <= LK_COORD_LIMIT && fabsf(gsx) <= LK_COORD_LIMIT && fabsf(gsy) <= LK_COORD_LIMIT)) {
        if (lane == 0) { o[0] = __float_as_uint(gsx); o[1] = __float_as_uint(gsy); o[2] = 0; o[3] = 0; }
        return;
    }
    const float halfx = (float)(ww - 1) * 0.5f, halfy = (float)(wh - 1) * 0.5f;
    const double area2 = (double)(2 * ww * wh), flt_scale = 1.0 / 1048576.0;
    const bool get_eig = (A.flags & LK_GET_MIN_EIGENVALS) != 0;
    float outx = 0.f, outy = 0.f, err = 0.f;
    int ok = 1;

    for (int lv = A.levels - 1; lv >= 0; lv--) {
        const int cols = L.cols[lv], rows = L.rows[lv];
        const uint8_t* __restrict__ I = L.prev[lv];
        const uint8_t* __restrict__ J = L.next[lv];
        const size_t si = L.prev_stride[lv], sj = L.next_stride[lv];
        const float scale = 1.f / (float)(1 << lv);
        float px = ptx * scale, py = pty * scale;
        float nx, ny;
        if (lv == A.levels - 1) { nx = gsx * scale; ny = gsy * scale; }      // (gs is the point itself without an initial guess)
        else { nx = outx * 2.f; ny = outy * 2.f; }
        outx = nx;
        outy = ny;
        px -= halfx;
        py -= halfy;
        const float fpx = floorf(px), fpy = floorf(py);
        if (!lk_in_range(fpx, fpy, ww, wh, cols, rows)) {
            if (lv == 0) { ok = 0; err = 0.f; }
            continue;
        }
        const int ix = (int)fpx, iy = (int)fpy;
        int w00, w01, w10, w11;
        lk_weights(px - fpx, py - fpy, w00, w01, w10, w11);

        __syncthreads();                                   // the level before has been read to its end
        for (int i = lane; i < pw * (wh + 3); i += LK_LANES) {
            const int y = i / pw, x = i - y * pw;
            s_patch[i] = I[(size_t)vp_lk_reflect(iy - 1 + y, rows) * si + vp_lk_reflect(ix - 1 + x, cols)];
        }
        __syncthreads();
        for (int i = lane; i < dw * (wh + 1); i += LK_LANES) {
            const int y = i / dw, x = i - y * dw;
            short2 d = make_short2(0, 0);
            if (ix + x >= 0 && ix + x < cols && iy + y >= 0 && iy + y < rows) {
                const uint8_t* p = s_patch + y * pw + x;       // the 3 x 3 neighbourhood's top-left corner
                const int t00 = 3 * (p[0] + p[2 * pw]) + 10 * p[pw], t02 = 3 * (p[2] + p[2 * pw + 2]) + 10 * p[pw + 2];
                const int t10 = p[2 * pw] - p[0], t11 = p[2 * pw + 1] - p[1], t12 = p[2 * pw + 2] - p[2];
                d = make_short2((short)(t02 - t00), (short)(3 * (t10 + t12) + 10 * t11));
            }
            s_deriv[i] = d;
        }
        __syncthreads();
        long long s11 = 0, s12 = 0, s22 = 0;
        {
            const int step_y = LK_LANES / ww, step_x = LK_LANES - step_y * ww;
            int x = lane % ww, y = lane / ww;
            for (int k = lane; k < area; k += LK_LANES) {
                const uint8_t* p = s_patch + (y + 1) * pw + x + 1;
                const short2 d00 = s_deriv[y * dw + x], d01 = s_deriv[y * dw + x + 1], d10 = s_deriv[(y + 1) * dw + x], d11 = s_deriv[(y + 1) * dw + x + 1];
                const int iv = lk_descale(p[0] * w00 + p[1] * w01 + p[pw] * w10 + p[pw + 1] * w11, LK_W_BITS - 5);
                const int gx = lk_descale(d00.x * w00 + d01.x * w01 + d10.x * w10 + d11.x * w11, LK_W_BITS);
                const int gy = lk_descale(d00.y * w00 + d01.y * w01 + d10.y * w10 + d11.y * w11, LK_W_BITS);
                s_I[k] = (int16_t)iv;
                s_Ix[k] = (int16_t)gx;
                s_Iy[k] = (int16_t)gy;
                s11 += gx * gx;
                s12 += gx * gy;
                s22 += gy * gy;
                x += step_x;
                y += step_y;
                if (x >= ww) { x -= ww; y++; }
            }
        }
        s11 = lk_wave_sum(s11);
        s12 = lk_wave_sum(s12);
        s22 = lk_wave_sum(s22);
        __syncthreads();

        const double A11 = (double)s11 * flt_scale, A12 = (double)s12 * flt_scale, A22 = (double)s22 * flt_scale;
        const double D = A11 * A22 - A12 * A12;
        const double dd = A11 - A22;
        const float min_eig = (float)(((A22 + A11) - __dsqrt_rn(dd * dd + 4.0 * (A12 * A12))) / area2);
        if (get_eig && lv == 0) err = min_eig;
        if ((double)min_eig < A.min_eig || D < (double)1.1920928955078125e-07f) {
            if (lv == 0) ok = 0;
            continue;
        }
        nx -= halfx;
        ny -= halfy;
        float pdx = 0.f, pdy = 0.f;
        for (int j = 0; j < A.max_count; j++) {
            const float fx = floorf(nx), fy = floorf(ny);
            if (!lk_in_range(fx, fy, ww, wh, cols, rows)) {
                if (lv == 0) ok = 0;
                break;
            }
            lk_weights(nx - fx, ny - fy, w00, w01, w10, w11);
            long long ib1, ib2;
            lk_mismatch(J, sj, cols, rows, (int)fx, (int)fy, w00, w01, w10, w11, ww, wh, s_I, s_Ix, s_Iy, 0, ib1, ib2);
            const double b1 = (double)ib1 * flt_scale, b2 = (double)ib2 * flt_scale;
            const float dx = (float)((A12 * b2 - A22 * b1) / D), dy = (float)((A12 * b1 - A11 * b2) / D);
            nx += dx;
            ny += dy;
            outx = nx + halfx;
            outy = ny + halfy;
            if ((double)dx * (double)dx + (double)dy * (double)dy <= A.eps2) break;
            if (j > 0 && fabs((double)(dx + pdx)) < 0.01 && fabs((double)(dy + pdy)) < 0.01) {
                outx -= dx * 0.5f;
                outy -= dy * 0.5f;
                break;
            }
            pdx = dx;
            pdy = dy;
        }
        if (ok && lv == 0 && !get_eig) {
            const float ex = outx - halfx, ey = outy - halfy, fx = floorf(ex), fy = floorf(ey);
            if (!lk_in_range(fx, fy, ww, wh, cols, rows)) ok = 0;
            else {
                lk_weights(ex - fx, ey - fy, w00, w01, w10, w11);
                long long sabs, unused;
                lk_mismatch(J, sj, cols, rows, (int)fx, (int)fy, w00, w01, w10, w11, ww, wh, s_I, s_Ix, s_Iy, 1, sabs, unused);
                err = (float)((double)sabs / (double)(32 * ww * wh));
            }
        }
    }
    if (lane == 0) {
        o[0] = __float_as_uint(outx);
        o[1] = __float_as_uint(outy);
        o[2] = (ok || get_eig) ? __float_as_uint(err) : 0u;
        o[3] = (u32)ok;
    }
}

int vpk_lk_flow(vp_ctx* ctx, const vp_lk_levels& L, const vp_lk_plan& P, int win_w, int win_h, int max_count, double eps2, int flags, double min_eig,
                const float* d_pts, const float* d_guess, u32* d_out)
{
    vp_lk_args A;
    A.win_w = win_w;
    A.win_h = win_h;
    A.levels = P.levels;
    A.max_count = max_count;
    A.flags = flags;
    A.off_deriv = (unsigned)P.off_deriv;
    A.off_win = (unsigned)P.off_win;
    A.eps2 = eps2;
    A.min_eig = min_eig;
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_lk_flow, dim3(P.grid), dim3(LK_LANES), P.lds_bytes, ctx->stream, L, A, d_pts, d_guess, d_out);
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
