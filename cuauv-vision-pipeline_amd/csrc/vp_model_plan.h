// Robust motion estimation from point pairs - cv2.findHomography, estimateAffine2D, estimateAffinePartial2D - as this library states
// it (vp_model.hip; the statement: tests/model_restate.py): the limits and argument checks, the counter-based
// sampler, the degeneracy tests, the three minimal solvers, the reprojection test, the stop table, the least-squares refit, the host
// form of the whole search and the plan of the device form.  Plain C++, a pure function of its arguments; what the kernels share is
// __host__ __device__.  Every double expression here is + - * / and comparisons in one written order, and the units that include
// this file are compiled without floating-point contraction, so device, host and the Python statement give the same bits.  libm
// appears in vp_rs_num_iters only, which the host alone calls.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/vp.h"

#ifdef __HIPCC__
#define VP_RS_HD __host__ __device__
#else
#define VP_RS_HD
#endif

#define RS_ROUND 256                 // hypotheses per round: one select block looks at them with one thread each
#define RS_STAGE 1024                // points a scoring block stages in LDS at once (16 bytes each)
#define RS_HYP_PER_BLOCK 16          // hypotheses a scoring block tests against its staged points, four waves taking turns
#define RS_THREADS 256
#define RS_MAX_POINTS (1 << 20)
#define RS_MAX_ITERS 65536
#define RS_MAX_ROUNDS (RS_MAX_ITERS / RS_ROUND)
#define RS_MAX_DRAWS 16              // draws a hypothesis may take to collect its distinct indices
#define RS_COLLINEAR_EPS 1.1920928955078125e-07   // FLT_EPSILON: three points are collinear when |cross| <= eps (|dx1| + |dy1| + |dx2| + |dy2|)
#define RS_PIVOT_MIN 1e-10           // the 8 x 8 elimination gives up on a pivot below it
#define RS_REFIT_EPS 1e-12           // the affine refit gives up when det <= eps Sxx Syy (the inliers lie on a line)

// what the device keeps between the launches of one call
struct vp_rs_state {
    int32_t done;                    // the search has ended: later launches return at once
    int32_t rounds;                  // rounds that counted
    int32_t best_count;              // -1: no valid hypothesis so far
    int32_t best_j;
    double best[9];
};

struct vp_rs_plan {
    int m;                           // points of a minimal sample
    int rounds;                      // at most this many, the last one cut at max_iters
    unsigned score_gx, score_gy;     // scoring: hypothesis groups x point chunks
    unsigned mask_grid;
    size_t off_need, off_counts, off_valid, off_models, off_state, off_mask, ws_bytes;   // behind the packed points at offset 0
};

VP_RS_HD static inline int vp_rs_sample_size(int model) { return model + 2; }
VP_RS_HD static inline double vp_rs_abs(double v) { return v < 0 ? -v : v; }
VP_RS_HD static inline bool vp_rs_finite(double v) { return v - v == 0.0; }

// NULL: admitted; else the reason (VP_ERR_INVALID).  What does not depend on pointers.
static inline const char* vp_rs_refusal(int n, int model, double threshold, int max_iters, double confidence)
{
    if (model < VP_MODEL_SIMILARITY || model > VP_MODEL_HOMOGRAPHY) return "motion model: unknown model";
    if (n < vp_rs_sample_size(model)) return "motion model: fewer point pairs than the model needs (2, 3 or 4)";
    if (n > RS_MAX_POINTS) return "motion model: at most 1048576 point pairs";
    if (!(threshold > 0) || !isfinite(threshold)) return "motion model: the threshold must be finite and above 0";
    if (max_iters < 1 || max_iters > RS_MAX_ITERS) return "motion model: max_iters must be 1 to 65536";
    if (!(confidence > 0 && confidence < 1)) return "motion model: the confidence must be above 0 and below 1";
    return nullptr;
}

// ---- sampling: draw d of hypothesis j under seed is a pure function of the three -----------------------------------------------------
VP_RS_HD static inline uint32_t vp_rs_mix(uint32_t x)      // lowbias32
{
    x ^= x >> 16;
    x *= 0x7feb352dU;
    x ^= x >> 15;
    x *= 0x846ca68bU;
    x ^= x >> 16;
    return x;
}

// the first m distinct indices among draws 0 .. RS_MAX_DRAWS - 1 -> s[0 .. m), the rest of s[0 .. 4) is -1; 0: fewer than m turned up
VP_RS_HD static inline int vp_rs_sample(int n, int m, uint32_t seed, uint32_t j, int32_t* s)
{
    const uint32_t key = vp_rs_mix(seed ^ (0x9e3779b9U * (j + 1U)));
    int got = 0;
    s[0] = s[1] = s[2] = s[3] = -1;
    for (uint32_t d = 0; d < RS_MAX_DRAWS && got < m; d++) {
        const int32_t idx = (int32_t)(((uint64_t)vp_rs_mix(key + d) * (uint64_t)(uint32_t)n) >> 32);
        bool seen = false;
        for (int k = 0; k < got; k++) seen = seen || s[k] == idx;
        if (!seen) s[got++] = idx;
    }
    return got == m;
}

// ---- degenerate samples --------------------------------------------------------------------------------------------------------------
// the cross product of (b - a) and (c - a) -> *cross; true when the three points count as collinear
VP_RS_HD static inline bool vp_rs_collinear(double ax, double ay, double bx, double by, double cx, double cy, double* cross)
{
    const double dx1 = bx - ax, dy1 = by - ay, dx2 = cx - ax, dy2 = cy - ay;
    const double cr = dx1 * dy2 - dy1 * dx2;
    *cross = cr;
    return !(vp_rs_abs(cr) > RS_COLLINEAR_EPS * (((vp_rs_abs(dx1) + vp_rs_abs(dy1)) + vp_rs_abs(dx2)) + vp_rs_abs(dy2)));
}

// ---- 8 x 8 elimination with partial pivoting (the first largest |pivot|), A and b destroyed; 0: a pivot below RS_PIVOT_MIN (or NaN) --
VP_RS_HD static inline int vp_rs_solve8(double A[8][8], double b[8], double g[8])
{
    for (int c = 0; c < 8; c++) {
        int piv = c;
        double amax = vp_rs_abs(A[c][c]);
        for (int r = c + 1; r < 8; r++) {
            const double a = vp_rs_abs(A[r][c]);
            if (a > amax) { amax = a; piv = r; }
        }
        if (!(amax >= RS_PIVOT_MIN)) return 0;
        if (piv != c) {
            for (int k = 0; k < 8; k++) { const double t = A[c][k]; A[c][k] = A[piv][k]; A[piv][k] = t; }
            const double t = b[c]; b[c] = b[piv]; b[piv] = t;
        }
        for (int r = c + 1; r < 8; r++) {
            const double f = A[r][c] / A[c][c];
            for (int k = c + 1; k < 8; k++) A[r][k] = A[r][k] - f * A[c][k];
            b[r] = b[r] - f * b[c];
        }
    }
    for (int c = 7; c >= 0; c--) {
        double s = b[c];
        for (int k = c + 1; k < 8; k++) s = s - A[c][k] * g[k];
        g[c] = s / A[c][c];
    }
    return 1;
}

// ---- hypothesis j: its sample and its model (H: nine doubles, row-major 3 x 3; zeros when void); 1 valid, 0 void -------------------
// src / dst: (x, y) float32 pairs `stride` floats apart (2: two plain arrays; 4: the packed form, dst = src + 2).  Both sets are
// shifted by the sample's first point before the solve, and the shift is folded back into H afterwards.
VP_RS_HD static inline int vp_rs_hypothesis(const float* src, const float* dst, size_t stride, int n, int model, uint32_t seed, uint32_t j, int32_t s[4], double H[9])
{
    const int m = vp_rs_sample_size(model);
    for (int k = 0; k < 9; k++) H[k] = 0.0;
    if (!vp_rs_sample(n, m, seed, j, s)) return 0;
    double px[4], py[4], qx[4], qy[4];
    for (int k = 0; k < m; k++) {
        px[k] = (double)src[(size_t)s[k] * stride];
        py[k] = (double)src[(size_t)s[k] * stride + 1];
        qx[k] = (double)dst[(size_t)s[k] * stride];
        qy[k] = (double)dst[(size_t)s[k] * stride + 1];
        if (!(vp_rs_finite(px[k]) && vp_rs_finite(py[k]) && vp_rs_finite(qx[k]) && vp_rs_finite(qy[k]))) return 0;
    }
    for (int a = 0; a < m; a++)
        for (int b = a + 1; b < m; b++)
            if ((px[a] == px[b] && py[a] == py[b]) || (qx[a] == qx[b] && qy[a] == qy[b])) return 0;
    double det = 0.0;                    // the source cross product of the sample's first triple
    if (m >= 3) {
        const int tri[4][3] = {{0, 1, 2}, {0, 1, 3}, {0, 2, 3}, {1, 2, 3}};
        const int ntri = m == 3 ? 1 : 4;
        int flips = 0;
        for (int t = 0; t < ntri; t++) {
            const int a = tri[t][0], b = tri[t][1], c = tri[t][2];
            double cs, cd;
            if (vp_rs_collinear(px[a], py[a], px[b], py[b], px[c], py[c], &cs)) return 0;
            if (vp_rs_collinear(qx[a], qy[a], qx[b], qy[b], qx[c], qy[c], &cd)) return 0;
            if (t == 0) det = cs;
            flips += (cs < 0) != (cd < 0);
        }
        if (model == VP_MODEL_HOMOGRAPHY && flips != 0 && flips != 4) return 0;
    }
    const double p0x = px[0], p0y = py[0], q0x = qx[0], q0y = qy[0];
    double R[9];
    if (model == VP_MODEL_SIMILARITY) {
        const double dx = px[1] - p0x, dy = py[1] - p0y, ex = qx[1] - q0x, ey = qy[1] - q0y;
        const double den = dx * dx + dy * dy;
        if (!(den > 0)) return 0;
        const double c = (dx * ex + dy * ey) / den, sn = (dx * ey - dy * ex) / den;
        R[0] = c; R[1] = -sn; R[2] = q0x - (c * p0x - sn * p0y);
        R[3] = sn; R[4] = c; R[5] = q0y - (sn * p0x + c * p0y);
        R[6] = 0.0; R[7] = 0.0; R[8] = 1.0;
    } else if (model == VP_MODEL_AFFINE) {
        const double a1x = px[1] - p0x, a1y = py[1] - p0y, a2x = px[2] - p0x, a2y = py[2] - p0y;
        const double b1x = qx[1] - q0x, b1y = qy[1] - q0y, b2x = qx[2] - q0x, b2y = qy[2] - q0y;
        const double m00 = (b1x * a2y - b2x * a1y) / det, m01 = (b2x * a1x - b1x * a2x) / det;
        const double m10 = (b1y * a2y - b2y * a1y) / det, m11 = (b2y * a1x - b1y * a2x) / det;
        R[0] = m00; R[1] = m01; R[2] = q0x - (m00 * p0x + m01 * p0y);
        R[3] = m10; R[4] = m11; R[5] = q0y - (m10 * p0x + m11 * p0y);
        R[6] = 0.0; R[7] = 0.0; R[8] = 1.0;
    } else {
        double A[8][8], b[8], g[8];
        for (int k = 0; k < 4; k++) {
            const double x = px[k] - p0x, y = py[k] - p0y, X = qx[k] - q0x, Y = qy[k] - q0y;
            double* r0 = A[2 * k];
            double* r1 = A[2 * k + 1];
            r0[0] = x; r0[1] = y; r0[2] = 1.0; r0[3] = 0.0; r0[4] = 0.0; r0[5] = 0.0; r0[6] = -(x * X); r0[7] = -(y * X);
            r1[0] = 0.0; r1[1] = 0.0; r1[2] = 0.0; r1[3] = x; r1[4] = y; r1[5] = 1.0; r1[6] = -(x * Y); r1[7] = -(y * Y);
            b[2 * k] = X;
            b[2 * k + 1] = Y;
        }
        if (!vp_rs_solve8(A, b, g)) return 0;
        const double c2 = g[2] - (g[0] * p0x + g[1] * p0y), c5 = g[5] - (g[3] * p0x + g[4] * p0y), c8 = 1.0 - (g[6] * p0x + g[7] * p0y);
        R[0] = g[0] + q0x * g[6]; R[1] = g[1] + q0x * g[7]; R[2] = c2 + q0x * c8;
        R[3] = g[3] + q0y * g[6]; R[4] = g[4] + q0y * g[7]; R[5] = c5 + q0y * c8;
        R[6] = g[6]; R[7] = g[7]; R[8] = c8;
    }
    for (int k = 0; k < 9; k++)
        if (!vp_rs_finite(R[k])) return 0;
    for (int k = 0; k < 9; k++) H[k] = R[k];
    return 1;
}

// ---- scoring: point (x, y) -> (X, Y) is an inlier of H iff its squared reprojection distance is <= t2 (false for NaN) ---------------
VP_RS_HD static inline bool vp_rs_inlier(const double* H, int model, double x, double y, double X, double Y, double t2)
{
    double u = (H[0] * x + H[1] * y) + H[2], v = (H[3] * x + H[4] * y) + H[5];
    if (model == VP_MODEL_HOMOGRAPHY) {
        const double w = (H[6] * x + H[7] * y) + H[8];
        u = u / w;
        v = v / w;
    }
    const double dx = u - X, dy = v - Y;
    return dx * dx + dy * dy <= t2;
}

// ---- how many hypotheses: cv2's RANSACUpdateNumIters(p, ep, m, max_iters), host only --------------------------------------------------
static inline int vp_rs_num_iters(double p, double ep, int m, int max_iters)
{
    p = p < 0 ? 0 : (p > 1 ? 1 : p);
    ep = ep < 0 ? 0 : (ep > 1 ? 1 : ep);
    double num = 1.0 - p;
    if (num < 2.2250738585072014e-308) num = 2.2250738585072014e-308;
    double denom = 1.0 - pow(1.0 - ep, (double)m);
    if (denom < 2.2250738585072014e-308) return 0;
    num = log(num);
    denom = log(denom);
    if (denom >= 0 || -num >= (double)max_iters * (-denom)) return max_iters;
    return (int)nearbyint(num / denom);
}

static inline int vp_rs_round_count(int max_iters) { return (max_iters + RS_ROUND - 1) / RS_ROUND; }

// need[r - 1], r = 1 .. rounds: the count the best hypothesis must have reached for the search to stop after round r - the smallest c
// in m .. n with num_iters(confidence, 1 - c / n) <= r RS_ROUND, found by bisection (the number falls as c grows, and is 0 at c = n)
static inline int vp_rs_stop_table(int n, int model, double confidence, int max_iters, int32_t* need)
{
    const int m = vp_rs_sample_size(model), rounds = vp_rs_round_count(max_iters);
    for (int r = 1; r <= rounds; r++) {
        int lo = m, hi = n;
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (vp_rs_num_iters(confidence, 1.0 - (double)mid / (double)n, m, max_iters) <= r * RS_ROUND) hi = mid;
            else lo = mid + 1;
        }
        need[r - 1] = lo;
    }
    return rounds;
}

// ---- the least-squares refit over the points whose mask byte is not 0 (mask NULL: all), sequentially in index order; 0: no model ---
static inline int vp_rs_refit(const float* src, const float* dst, size_t stride, int n, const uint8_t* mask, int model, double H[9])
{
    for (int k = 0; k < 9; k++) H[k] = 0.0;
    int cnt = 0;
    double spx = 0, spy = 0, sqx = 0, sqy = 0;
    for (int i = 0; i < n; i++) {
        if (mask && !mask[i]) continue;
        cnt++;
        spx = spx + (double)src[i * stride];
        spy = spy + (double)src[i * stride + 1];
        sqx = sqx + (double)dst[i * stride];
        sqy = sqy + (double)dst[i * stride + 1];
    }
    if (cnt < vp_rs_sample_size(model)) return 0;
    const double k = (double)cnt, cpx = spx / k, cpy = spy / k, cqx = sqx / k, cqy = sqy / k;
    double R[9];
    if (model == VP_MODEL_SIMILARITY) {
        double Sxx = 0, Sa = 0, Sb = 0;
        for (int i = 0; i < n; i++) {
            if (mask && !mask[i]) continue;
            const double dx = (double)src[i * stride] - cpx, dy = (double)src[i * stride + 1] - cpy;
            const double ex = (double)dst[i * stride] - cqx, ey = (double)dst[i * stride + 1] - cqy;
            Sxx = Sxx + (dx * dx + dy * dy);
            Sa = Sa + (dx * ex + dy * ey);
            Sb = Sb + (dx * ey - dy * ex);
        }
        if (!(Sxx > 0)) return 0;
        const double a = Sa / Sxx, b = Sb / Sxx;
        R[0] = a; R[1] = -b; R[2] = cqx - (a * cpx - b * cpy);
        R[3] = b; R[4] = a; R[5] = cqy - (b * cpx + a * cpy);
        R[6] = 0.0; R[7] = 0.0; R[8] = 1.0;
    } else if (model == VP_MODEL_AFFINE) {
        double Sxx = 0, Sxy = 0, Syy = 0, SxX = 0, SyX = 0, SxY = 0, SyY = 0;
        for (int i = 0; i < n; i++) {
            if (mask && !mask[i]) continue;
            const double dx = (double)src[i * stride] - cpx, dy = (double)src[i * stride + 1] - cpy;
            const double ex = (double)dst[i * stride] - cqx, ey = (double)dst[i * stride + 1] - cqy;
            Sxx = Sxx + dx * dx;
            Sxy = Sxy + dx * dy;
            Syy = Syy + dy * dy;
            SxX = SxX + dx * ex;
            SyX = SyX + dy * ex;
            SxY = SxY + dx * ey;
            SyY = SyY + dy * ey;
        }
        const double det = Sxx * Syy - Sxy * Sxy;
        if (!(det > RS_REFIT_EPS * (Sxx * Syy))) return 0;
        const double m00 = (SxX * Syy - SyX * Sxy) / det, m01 = (SyX * Sxx - SxX * Sxy) / det;
        const double m10 = (SxY * Syy - SyY * Sxy) / det, m11 = (SyY * Sxx - SxY * Sxy) / det;
        R[0] = m00; R[1] = m01; R[2] = cqx - (m00 * cpx + m01 * cpy);
        R[3] = m10; R[4] = m11; R[5] = cqy - (m10 * cpx + m11 * cpy);
        R[6] = 0.0; R[7] = 0.0; R[8] = 1.0;
    } else {
        // Hartley's normalisation in cv2's form: each set is centred, and each axis scaled to a mean absolute deviation of 1
        double apx = 0, apy = 0, aqx = 0, aqy = 0;
        for (int i = 0; i < n; i++) {
            if (mask && !mask[i]) continue;
            apx = apx + vp_rs_abs((double)src[i * stride] - cpx);
            apy = apy + vp_rs_abs((double)src[i * stride + 1] - cpy);
            aqx = aqx + vp_rs_abs((double)dst[i * stride] - cqx);
            aqy = aqy + vp_rs_abs((double)dst[i * stride + 1] - cqy);
        }
        if (!(apx > 0 && apy > 0 && aqx > 0 && aqy > 0)) return 0;
        const double s1x = k / apx, s1y = k / apy, s2x = k / aqx, s2y = k / aqy;
        double A[8][8], b[8], g[8];
        for (int r = 0; r < 8; r++) {
            b[r] = 0.0;
            for (int c = 0; c < 8; c++) A[r][c] = 0.0;
        }
        // the normal equations of the two rows a point contributes (h33 = 1): the upper triangle, row by row, first row first
        for (int i = 0; i < n; i++) {
            if (mask && !mask[i]) continue;
            const double x = ((double)src[i * stride] - cpx) * s1x, y = ((double)src[i * stride + 1] - cpy) * s1y;
            const double X = ((double)dst[i * stride] - cqx) * s2x, Y = ((double)dst[i * stride + 1] - cqy) * s2y;
            const double r0[8] = {x, y, 1.0, 0.0, 0.0, 0.0, -(x * X), -(y * X)};
            const double r1[8] = {0.0, 0.0, 0.0, x, y, 1.0, -(x * Y), -(y * Y)};
            for (int r = 0; r < 8; r++) {
                for (int c = r; c < 8; c++) {
                    A[r][c] = A[r][c] + r0[r] * r0[c];
                    A[r][c] = A[r][c] + r1[r] * r1[c];
                }
                b[r] = b[r] + r0[r] * X;
                b[r] = b[r] + r1[r] * Y;
            }
        }
        for (int r = 0; r < 8; r++)
            for (int c = 0; c < r; c++) A[r][c] = A[c][r];
        if (!vp_rs_solve8(A, b, g)) return 0;
        // H = T2^-1 G T1, then divided by its last entry
        const double e0 = g[0] * s1x, e1 = g[1] * s1y, e2 = g[2] - (e0 * cpx + e1 * cpy);
        const double e3 = g[3] * s1x, e4 = g[4] * s1y, e5 = g[5] - (e3 * cpx + e4 * cpy);
        const double e6 = g[6] * s1x, e7 = g[7] * s1y, e8 = 1.0 - (e6 * cpx + e7 * cpy);
        const double f0 = e0 / s2x + cqx * e6, f1 = e1 / s2x + cqx * e7, f2 = e2 / s2x + cqx * e8;
        const double f3 = e3 / s2y + cqy * e6, f4 = e4 / s2y + cqy * e7, f5 = e5 / s2y + cqy * e8;
        if (!vp_rs_finite(e8) || e8 == 0) return 0;
        R[0] = f0 / e8; R[1] = f1 / e8; R[2] = f2 / e8;
        R[3] = f3 / e8; R[4] = f4 / e8; R[5] = f5 / e8;
        R[6] = e6 / e8; R[7] = e7 / e8; R[8] = e8 / e8;
    }
    for (int i = 0; i < 9; i++)
        if (!vp_rs_finite(R[i])) return 0;
    for (int i = 0; i < 9; i++) H[i] = R[i];
    return 1;
}

// ---- the whole search on the host: the statement as a loop over the functions above --------------------------------------------------
// need: the stop table of `rounds` entries.  mask (n bytes) and H receive the answer; returns the inlier count, 0 when there is no
// model (mask and H are zeros then).  *n_hyp: hypotheses taken.
static inline int vp_rs_search_host(const float* src, const float* dst, size_t stride, int n, int model, double t2, int max_iters, const int32_t* need, int rounds,
                                    uint32_t seed, double H[9], uint8_t* mask, int* n_hyp)
{
    const int m = vp_rs_sample_size(model);
    int best = -1, taken = 0;
    double B[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, T[9];
    int32_t s[4];
    for (int r = 0; r < rounds; r++) {
        const int end = (r + 1) * RS_ROUND < max_iters ? (r + 1) * RS_ROUND : max_iters;
        for (int j = r * RS_ROUND; j < end; j++) {
            if (!vp_rs_hypothesis(src, dst, stride, n, model, seed, (uint32_t)j, s, T)) continue;
            int c = 0;
            for (int i = 0; i < n; i++)
                c += vp_rs_inlier(T, model, (double)src[i * stride], (double)src[i * stride + 1], (double)dst[i * stride], (double)dst[i * stride + 1], t2);
            if (c > best) {
                best = c;
                for (int k = 0; k < 9; k++) B[k] = T[k];
            }
        }
        taken = end;
        if (best >= need[r]) break;
    }
    *n_hyp = taken;
    int c = 0;
    for (int i = 0; i < n; i++) {
        mask[i] = best >= m && vp_rs_inlier(B, model, (double)src[i * stride], (double)src[i * stride + 1], (double)dst[i * stride], (double)dst[i * stride + 1], t2);
        c += mask[i];
    }
    if (best < m || !vp_rs_refit(src, dst, stride, n, mask, model, H)) {
        for (int i = 0; i < n; i++) mask[i] = 0;
        for (int k = 0; k < 9; k++) H[k] = 0.0;
        return 0;
    }
    return c;
}

// ---- the plan of the device form; arguments as vp_rs_refusal admitted them ------------------------------------------------------------
static inline size_t vp_rs_align(size_t v) { return (v + 255) / 256 * 256; }
static inline void vp_rs_make_plan(int n, int model, int max_iters, vp_rs_plan* P)
{
    P->m = vp_rs_sample_size(model);
    P->rounds = vp_rs_round_count(max_iters);
    P->score_gx = RS_ROUND / RS_HYP_PER_BLOCK;
    P->score_gy = (unsigned)((n + RS_STAGE - 1) / RS_STAGE);
    P->mask_grid = (unsigned)((n + RS_THREADS - 1) / RS_THREADS);
    P->off_need = vp_rs_align((size_t)n * 16);
    P->off_counts = P->off_need + vp_rs_align((size_t)P->rounds * 4);
    P->off_valid = P->off_counts + vp_rs_align(RS_ROUND * 4);
    P->off_models = P->off_valid + vp_rs_align(RS_ROUND * 4);
    P->off_state = P->off_models + vp_rs_align(RS_ROUND * 9 * 8);
    P->off_mask = P->off_state + vp_rs_align(sizeof(vp_rs_state));
    P->ws_bytes = P->off_mask + vp_rs_align((size_t)n);
}

static_assert(VP_MODEL_SIMILARITY == 0 && VP_MODEL_AFFINE == 1 && VP_MODEL_HOMOGRAPHY == 2, "motion model: the sample size is model + 2");
static_assert(RS_ROUND == RS_THREADS && RS_ROUND <= 256, "motion model: the select block has one thread per hypothesis and packs its index into 8 bits");
static_assert(((unsigned long long)(RS_MAX_POINTS + 1) << 8) + 255 < (1ull << 32), "motion model: count + 1 and the index share a 32-bit key");
static_assert(RS_ROUND % RS_HYP_PER_BLOCK == 0 && RS_HYP_PER_BLOCK % (RS_THREADS / 64) == 0, "motion model: the waves of a block take equal turns");
static_assert(RS_STAGE * 16 <= 65536, "motion model: the staged points fit the LDS a kernel gets without asking");
static_assert((RS_MAX_POINTS + RS_STAGE - 1) / RS_STAGE <= 65535, "motion model: the chunks fit the grid's y extent");
static_assert(RS_MAX_ITERS % RS_ROUND == 0 && (long long)RS_MAX_ROUNDS * RS_ROUND < (1ll << 31), "motion model: r RS_ROUND stays an int");
static_assert(RS_MAX_DRAWS >= 4, "motion model: a homography sample needs four draws at least");
