// Robust rigid 3-D motion q = R p + t between paired 3-D points as this library states it (vp_rigid.hip; the
// statement: tests/rigid_restate.py): the limits and argument checks, the pair of a track, the hypothesis from three pairs, the two
// inlier tests, the refit from the seventeen sums, the host form of the whole search and the plan of the device form.  The mixer and
// the sampler are those of vp_model_plan.h; the point test, the collinearity bound and the stop rule are those of vp_plane_plan.h.
// Plain C++, a pure function of its arguments; what the kernels share is __host__ __device__.  Every double expression of the search
// is + - * / sqrt and comparisons in one written order, and the units that include this file are compiled without floating-point
// contraction, so device, host and the Python statement give the same bits.
#pragma once
#include "vp_plane_plan.h"

#define RG_RUN 1024                  // candidates a compaction block counts and ranks: four passes of its 256 threads
#define RG_STAGE RS_STAGE            // pairs a scoring block stages in LDS at once (32 bytes each)
#define RG_HYP_PER_BLOCK RS_HYP_PER_BLOCK
#define RG_THREADS RS_THREADS
#define RG_MAX_PAIRS RS_MAX_POINTS
#define RG_MAX_SIDE 4096
#define RG_MOTION 12                 // R row-major and t
#define RG_MODEL 18                  // doubles kept per hypothesis: the motion and the sample's first pair (p0, q0)
#define RG_SUMS 17                   // sum u (3), sum v (3), sum u v^T (9, row-major), sum |u|^2, sum |v|^2; u = p - p0, v = q - q0
#define RG_REFIT_EPS 1e-12           // the refit is degenerate unless the two largest eigenvalues differ by more than this times the largest
#define RG_JACOBI_SWEEPS 12

// what the device keeps between the launches of one call
struct vp_rg_state {
    int32_t done;                    // the search has ended: later launches return at once
    int32_t rounds;                  // rounds that counted
    int32_t best_count;              // -1: no valid hypothesis so far
    int32_t best_j;
    int32_t n_usable;                // written by the scan, read by everything after it
    int32_t pad;
    double best[RG_MODEL];
    double sums[RG_SUMS];
};

// the inlier test's constants: t2 = T T, fb = focal_px baseline
struct vp_rg_metric { int metric; double t2, f, fb; };

struct vp_rg_plan {
    int n;                           // pairs or tracks given: the most usable pairs there can be
    int rounds;
    unsigned runs;                   // compaction blocks
    unsigned score_gx, score_gy;     // scoring: hypothesis groups x pair chunks (of the most pairs there can be)
    unsigned finish_grid;
};

// the buffers of a call inside the context's workspace
struct vp_rg_buffers {
    float* pairs;                    // n times two float4: p and the original index, q and padding
    int32_t* run_count; int32_t* run_off;
    double* qcrit;                   // per round: the smallest ratio best / n at which the search stops (vp_pl_stop_ratios)
    int32_t* counts; int32_t* valid; double* models;
    vp_rg_state* state;
};

static inline void vp_rg_declare(vp_ws_frame& W, const vp_rg_plan& P, vp_rg_buffers* B)
{
    W.want(&B->pairs, (size_t)P.n * 32);
    W.want(&B->run_count, (size_t)P.runs * 4);
    W.want(&B->run_off, (size_t)P.runs * 4);
    W.want(&B->qcrit, (size_t)P.rounds * 8);
    W.want(&B->counts, RS_ROUND * 4);
    W.want(&B->valid, RS_ROUND * 4);
    W.want(&B->models, RS_ROUND * RG_MODEL * 8);
    W.want(&B->state, sizeof(vp_rg_state));
}

// NULL: admitted; else the reason (VP_ERR_INVALID).  What does not depend on pointers.
static inline const char* vp_rg_count_refusal(int n)
{
    if (n < 1 || n > RG_MAX_PAIRS) return "fit rigid: 1 to 1048576 pairs";
    return nullptr;
}

static inline const char* vp_rg_size_refusal(int w, int h)
{
    if (w < 1 || w > RG_MAX_SIDE || h < 1 || h > RG_MAX_SIDE) return "fit rigid: the images must be 1 to 4096 pixels wide and high";
    return nullptr;
}

// focal_px and baseline count under VP_RIGID_DISPARITY only
static inline const char* vp_rg_search_refusal(int metric, double threshold, double focal_px, double baseline, int max_iters, double confidence)
{
    if (metric != VP_RIGID_EUCLID && metric != VP_RIGID_DISPARITY) return "fit rigid: unknown metric";
    if (!(threshold > 0) || !isfinite(threshold)) return "fit rigid: the threshold must be finite and above 0";
    if (metric == VP_RIGID_DISPARITY) {
        if (!(focal_px > 0) || !isfinite(focal_px)) return "fit rigid: focal_px must be finite and above 0";
        if (!(baseline > 0) || !isfinite(baseline)) return "fit rigid: the baseline must be finite and above 0";
    }
    if (max_iters < 1 || max_iters > RS_MAX_ITERS) return "fit rigid: max_iters must be 1 to 65536";
    if (!(confidence > 0 && confidence < 1)) return "fit rigid: the confidence must be above 0 and below 1";
    return nullptr;
}

static inline vp_rg_metric vp_rg_make_metric(int metric, double threshold, double focal_px, double baseline)
{
    const bool d = metric == VP_RIGID_DISPARITY;
    return vp_rg_metric{metric, threshold * threshold, d ? focal_px : 0.0, d ? focal_px * baseline : 0.0};
}

static inline void vp_rg_make_plan(int n, int max_iters, vp_rg_plan* P)
{
    P->n = n;
    P->rounds = vp_rs_round_count(max_iters);
    P->runs = (unsigned)((n + RG_RUN - 1) / RG_RUN);
    P->score_gx = RS_ROUND / RG_HYP_PER_BLOCK;
    P->score_gy = (unsigned)((n + RG_STAGE - 1) / RG_STAGE);
    P->finish_grid = (unsigned)((n + RG_THREADS - 1) / RG_THREADS);
}

// ---- the pair of a track -----------------------------------------------------------------------------------------------------------------
struct vp_rg_tracks {
    const float* xyz0; size_t stride0;       // the previous frame's points, rows of stride0 bytes
    const float* xyz1; size_t stride1;       // the current frame's
    int w, h;
    const float* prev;                       // n (x, y)
    const uint32_t* rows;                    // n rows of x, y, err (float32 bits) and status
};

// the nearest pixel of a coordinate: ix = floor(x + 0.5f), admitted iff x >= -0.5f && x < extent - 0.5f (false for NaN)
VP_RS_HD static inline bool vp_rg_pixel(float x, int extent, int* ix)
{
    if (!(x >= -0.5f && x < (float)extent - 0.5f)) return false;
    int i = (int)floorf(x + 0.5f);
    if (i > extent - 1) i = extent - 1;      // the sum cannot round up to the extent below 2^23; a bound on the read all the same
    if (i < 0) i = 0;
    *ix = i;
    return true;
}

VP_RS_HD static inline float vp_rg_bits(uint32_t v)
{
    union { uint32_t u; float f; } c;
    c.u = v;
    return c.f;
}

// track i -> p (previous frame) and q (current frame); false when it gives no pair
VP_RS_HD static inline bool vp_rg_track_pair(const vp_rg_tracks& T, int i, float p[3], float q[3])
{
    const uint32_t* row = T.rows + (size_t)i * 4;
    if (row[3] == 0) return false;
    const float x0 = T.prev[(size_t)i * 2], y0 = T.prev[(size_t)i * 2 + 1], x1 = vp_rg_bits(row[0]), y1 = vp_rg_bits(row[1]);
    if (!(x0 - x0 == 0.0f && y0 - y0 == 0.0f && x1 - x1 == 0.0f && y1 - y1 == 0.0f)) return false;
    int ix0, iy0, ix1, iy1;
    if (!vp_rg_pixel(x0, T.w, &ix0) || !vp_rg_pixel(y0, T.h, &iy0) || !vp_rg_pixel(x1, T.w, &ix1) || !vp_rg_pixel(y1, T.h, &iy1)) return false;
    const float* a = reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(T.xyz0) + (size_t)iy0 * T.stride0) + 3 * (size_t)ix0;
    const float* b = reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(T.xyz1) + (size_t)iy1 * T.stride1) + 3 * (size_t)ix1;
    p[0] = a[0]; p[1] = a[1]; p[2] = a[2];
    q[0] = b[0]; q[1] = b[1]; q[2] = b[2];
    return vp_pl_usable(p[0], p[1], p[2]) && vp_pl_usable(q[0], q[1], q[2]);
}

// ---- the motion through three pairs; 1 valid, 0 void ---------------------------------------------------------------------------------------
// the orthonormal frame of a triad: u1 along e1, u3 along e1 x e2, u2 = u3 x u1 -> F[3][3] (rows u1 u2 u3); 0: the triad is collinear
VP_RS_HD static inline int vp_rg_frame(const double* p0, const double* p1, const double* p2, double F[3][3])
{
    const double e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
    const double e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
    const double c0 = (e1y * e2z) - (e1z * e2y);
    const double c1 = (e1z * e2x) - (e1x * e2z);
    const double c2 = (e1x * e2y) - (e1y * e2x);
    const double l2 = ((c0 * c0) + (c1 * c1)) + (c2 * c2);
    const double a = ((e1x * e1x) + (e1y * e1y)) + (e1z * e1z);
    const double b = ((e2x * e2x) + (e2y * e2y)) + (e2z * e2z);
    if (!(l2 > PL_VOID_SIN2 * (a * b))) return 0;
    const double la = vp_pl_sqrt(a), lc = vp_pl_sqrt(l2);
    F[0][0] = e1x / la; F[0][1] = e1y / la; F[0][2] = e1z / la;
    F[2][0] = c0 / lc; F[2][1] = c1 / lc; F[2][2] = c2 / lc;
    F[1][0] = (F[2][1] * F[0][2]) - (F[2][2] * F[0][1]);
    F[1][1] = (F[2][2] * F[0][0]) - (F[2][0] * F[0][2]);
    F[1][2] = (F[2][0] * F[0][1]) - (F[2][1] * F[0][0]);
    return 1;
}

// p[3][3], q[3][3]: the three pairs -> M[0 .. 12): R row-major and t
VP_RS_HD static inline int vp_rg_motion_from(const double p[3][3], const double q[3][3], double* M)
{
    double U[3][3], V[3][3];
    if (!vp_rg_frame(p[0], p[1], p[2], U)) return 0;
    if (!vp_rg_frame(q[0], q[1], q[2], V)) return 0;
    double R[9], t[3], cp[3], cq[3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) R[r * 3 + c] = ((V[0][r] * U[0][c]) + (V[1][r] * U[1][c])) + (V[2][r] * U[2][c]);
    for (int c = 0; c < 3; c++) {
        cp[c] = ((p[0][c] + p[1][c]) + p[2][c]) / 3.0;
        cq[c] = ((q[0][c] + q[1][c]) + q[2][c]) / 3.0;
    }
    for (int r = 0; r < 3; r++) t[r] = cq[r] - (((R[r * 3] * cp[0]) + (R[r * 3 + 1] * cp[1])) + (R[r * 3 + 2] * cp[2]));
    for (int k = 0; k < 9; k++)
        if (!vp_rs_finite(R[k])) return 0;
    for (int k = 0; k < 3; k++)
        if (!vp_rs_finite(t[k])) return 0;
    for (int k = 0; k < 9; k++) M[k] = R[k];
    for (int k = 0; k < 3; k++) M[9 + k] = t[k];
    return 1;
}

// hypothesis j over n pairs: src / dst are (x, y, z) float32 triples `stride` floats apart (3: two plain arrays; 8: the packed form,
// dst = src + 4): its sample -> s[0 .. 3), its RG_MODEL doubles -> M (zeros when void)
VP_RS_HD static inline int vp_rg_hypothesis(const float* src, const float* dst, size_t stride, int n, uint32_t seed, uint32_t j, int32_t s[4], double M[RG_MODEL])
{
    for (int k = 0; k < RG_MODEL; k++) M[k] = 0.0;
    if (!vp_rs_sample(n, 3, seed, j, s)) return 0;
    double p[3][3], q[3][3];
    for (int k = 0; k < 3; k++)
        for (int c = 0; c < 3; c++) {
            p[k][c] = (double)src[(size_t)s[k] * stride + c];
            q[k][c] = (double)dst[(size_t)s[k] * stride + c];
        }
    double T[RG_MOTION];
    if (!vp_rg_motion_from(p, q, T)) return 0;
    for (int k = 0; k < RG_MOTION; k++) M[k] = T[k];
    for (int c = 0; c < 3; c++) { M[12 + c] = p[0][c]; M[15 + c] = q[0][c]; }
    return 1;
}

// ---- the inlier test ---------------------------------------------------------------------------------------------------------------------
// what the test needs of the destination point: under VP_RIGID_DISPARITY its three terms do not depend on the hypothesis, so a
// scoring wave forms them once per pair; the expressions are the statement's either way
struct vp_rg_dst { double x, y, z, a, b, c; bool ok; };

VP_RS_HD static inline vp_rg_dst vp_rg_dst_side(const vp_rg_metric& K, double qx, double qy, double qz)
{
    vp_rg_dst D = {qx, qy, qz, 0.0, 0.0, 0.0, true};
    if (K.metric == VP_RIGID_DISPARITY) {
        D.ok = qz > 0;
        if (D.ok) { D.a = qx / qz; D.b = qy / qz; D.c = 1.0 / qz; }
    }
    return D;
}

VP_RS_HD static inline bool vp_rg_inlier(const double* M, const vp_rg_metric& K, double x, double y, double z, const vp_rg_dst& D)
{
    const double mx = (((M[0] * x) + (M[1] * y)) + (M[2] * z)) + M[9];
    const double my = (((M[3] * x) + (M[4] * y)) + (M[5] * z)) + M[10];
    const double mz = (((M[6] * x) + (M[7] * y)) + (M[8] * z)) + M[11];
    if (K.metric == VP_RIGID_DISPARITY) {
        if (!D.ok || !(mz > 0)) return false;
        const double du = K.f * ((mx / mz) - D.a), dv = K.f * ((my / mz) - D.b), dd = K.fb * ((1.0 / mz) - D.c);
        return ((du * du) + (dv * dv)) + (dd * dd) <= K.t2;
    }
    const double dx = mx - D.x, dy = my - D.y, dz = mz - D.z;
    return ((dx * dx) + (dy * dy)) + (dz * dz) <= K.t2;
}

// pair i of the packed form
VP_RS_HD static inline bool vp_rg_inlier_packed(const double* M, const vp_rg_metric& K, const float* pairs, int i)
{
    const float* e = pairs + (size_t)i * 8;
    return vp_rg_inlier(M, K, (double)e[0], (double)e[1], (double)e[2], vp_rg_dst_side(K, (double)e[4], (double)e[5], (double)e[6]));
}

// ---- the refit from the count and the seventeen sums about (p0, q0) -> result[31] -------------------------------------------------------------
// cyclic Jacobi on a symmetric 4 x 4: eigenvalues on A's diagonal, eigenvectors in V's columns
static inline void vp_rg_jacobi4(double A[4][4], double V[4][4])
{
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) V[r][c] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < RG_JACOBI_SWEEPS; sweep++)
        for (int p = 0; p < 3; p++)
            for (int q = p + 1; q < 4; q++) {
                const double apq = A[p][q];
                if (apq == 0.0 || !vp_rs_finite(apq)) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                double t = 1.0 / (vp_rs_abs(theta) + sqrt((theta * theta) + 1.0));
                if (theta < 0) t = -t;
                const double c = 1.0 / sqrt((t * t) + 1.0), s = t * c;
                const double app = A[p][p], aqq = A[q][q];
                A[p][p] = app - (t * apq);
                A[q][q] = aqq + (t * apq);
                A[p][q] = A[q][p] = 0.0;
                for (int r = 0; r < 4; r++) {
                    if (r == p || r == q) continue;
                    const double arp = A[r][p], arq = A[r][q];
                    A[r][p] = A[p][r] = (c * arp) - (s * arq);
                    A[r][q] = A[q][r] = (s * arp) + (c * arq);
                }
                for (int k = 0; k < 4; k++) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = (c * vkp) - (s * vkq);
                    V[k][q] = (s * vkp) + (c * vkq);
                }
            }
}

// the rms residual of the motion M over the summed pairs: r_i = (R u_i - v_i) + e0, e0 = (R p0 + t) - q0
static inline double vp_rg_rms(int k, const double* S, const double* p0, const double* q0, const double* M)
{
    const double kk = (double)k;
    double e0[3], Rsu[3], cross = 0.0;
    for (int r = 0; r < 3; r++) {
        e0[r] = ((((M[r * 3] * p0[0]) + (M[r * 3 + 1] * p0[1])) + (M[r * 3 + 2] * p0[2])) + M[9 + r]) - q0[r];
        Rsu[r] = ((M[r * 3] * S[0]) + (M[r * 3 + 1] * S[1])) + (M[r * 3 + 2] * S[2]);
        for (int c = 0; c < 3; c++) cross = cross + (M[r * 3 + c] * S[6 + c * 3 + r]);
    }
    double ss = (S[15] + S[16]) - (2.0 * cross);             // |R u| = |u|: R is a rotation
    ss = ss + (2.0 * ((((e0[0] * Rsu[0]) + (e0[1] * Rsu[1])) + (e0[2] * Rsu[2])) - (((e0[0] * S[3]) + (e0[1] * S[4])) + (e0[2] * S[5]))));
    ss = ss + (kk * (((e0[0] * e0[0]) + (e0[1] * e0[1])) + (e0[2] * e0[2])));
    const double rms = sqrt((ss > 0 ? ss : 0.0) / kk);
    return vp_rs_finite(rms) ? rms : 0.0;
}

// best: the best hypothesis (RG_MOTION doubles), or NULL for the refit alone.  Returns 1; 0 (zeros) when there are fewer than three
// pairs, or when the refit is degenerate and there is no hypothesis to fall back to.
static inline int vp_rg_refit_close(int k, const double* S, const double* p0, const double* q0, const double* best, double* result)
{
    for (int i = 0; i < VP_RIGID_RESULT; i++) result[i] = 0.0;
    if (k < 3) return 0;
    const double kk = (double)k;
    double cp[3], cq[3], C[3][3];
    for (int c = 0; c < 3; c++) { cp[c] = p0[c] + (S[c] / kk); cq[c] = q0[c] + (S[3 + c] / kk); }
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) C[r][c] = S[6 + r * 3 + c] - ((S[r] * S[3 + c]) / kk);
    // Horn's matrix: its largest eigenvector is the quaternion (w, x, y, z) of the rotation that carries the p side onto the q side
    double N[4][4], V[4][4];
    N[0][0] = (C[0][0] + C[1][1]) + C[2][2];
    N[1][1] = (C[0][0] - C[1][1]) - C[2][2];
    N[2][2] = (C[1][1] - C[0][0]) - C[2][2];
    N[3][3] = (C[2][2] - C[0][0]) - C[1][1];
    N[0][1] = N[1][0] = C[1][2] - C[2][1];
    N[0][2] = N[2][0] = C[2][0] - C[0][2];
    N[0][3] = N[3][0] = C[0][1] - C[1][0];
    N[1][2] = N[2][1] = C[0][1] + C[1][0];
    N[1][3] = N[3][1] = C[2][0] + C[0][2];
    N[2][3] = N[3][2] = C[1][2] + C[2][1];
    vp_rg_jacobi4(N, V);
    int hi = 0;
    for (int i = 1; i < 4; i++) if (N[i][i] > N[hi][hi]) hi = i;
    int second = hi == 0 ? 1 : 0;
    for (int i = 0; i < 4; i++) if (i != hi && N[i][i] > N[second][second]) second = i;
    double M[RG_MOTION];
    bool ok = N[hi][hi] - N[second][second] > RG_REFIT_EPS * vp_rs_abs(N[hi][hi]);     // else the inliers lie on a line (or are one point)
    if (ok) {
        double w = V[0][hi], x = V[1][hi], y = V[2][hi], z = V[3][hi];
        const double len = sqrt((((w * w) + (x * x)) + (y * y)) + (z * z));
        w = w / len; x = x / len; y = y / len; z = z / len;
        M[0] = (((w * w) + (x * x)) - (y * y)) - (z * z); M[1] = 2.0 * ((x * y) - (w * z)); M[2] = 2.0 * ((x * z) + (w * y));
        M[3] = 2.0 * ((x * y) + (w * z)); M[4] = (((w * w) - (x * x)) + (y * y)) - (z * z); M[5] = 2.0 * ((y * z) - (w * x));
        M[6] = 2.0 * ((x * z) - (w * y)); M[7] = 2.0 * ((y * z) + (w * x)); M[8] = (((w * w) - (x * x)) - (y * y)) + (z * z);
        for (int r = 0; r < 3; r++) M[9 + r] = cq[r] - (((M[r * 3] * cp[0]) + (M[r * 3 + 1] * cp[1])) + (M[r * 3 + 2] * cp[2]));
        for (int i = 0; i < RG_MOTION; i++) ok = ok && vp_rs_finite(M[i]);
    }
    if (!ok) {
        if (!best) return 0;
        for (int i = 0; i < RG_MOTION; i++) M[i] = best[i];      // the best hypothesis stands
    }
    for (int i = 0; i < RG_MOTION; i++) result[i] = M[i];
    if (best)
        for (int i = 0; i < RG_MOTION; i++) result[12 + i] = best[i];
    for (int c = 0; c < 3; c++) { result[24 + c] = cp[c]; result[27 + c] = cq[c]; }
    result[30] = vp_rg_rms(k, S, p0, q0, M);
    return 1;
}

// the count and the seventeen sums over the pairs whose keep byte is not 0 (keep NULL: all), in index order; src / dst / stride as
// vp_rg_hypothesis takes them
static inline int vp_rg_sums_host(const float* src, const float* dst, size_t stride, int n, const uint8_t* keep, const double* p0, const double* q0, double* S)
{
    int k = 0;
    for (int i = 0; i < RG_SUMS; i++) S[i] = 0.0;
    for (int i = 0; i < n; i++) {
        if (keep && !keep[i]) continue;
        double u[3], v[3];
        for (int c = 0; c < 3; c++) { u[c] = (double)src[(size_t)i * stride + c] - p0[c]; v[c] = (double)dst[(size_t)i * stride + c] - q0[c]; }
        k++;
        for (int c = 0; c < 3; c++) { S[c] = S[c] + u[c]; S[3 + c] = S[3 + c] + v[c]; }
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) S[6 + r * 3 + c] = S[6 + r * 3 + c] + (u[r] * v[c]);
        S[15] = S[15] + (((u[0] * u[0]) + (u[1] * u[1])) + (u[2] * u[2]));
        S[16] = S[16] + (((v[0] * v[0]) + (v[1] * v[1])) + (v[2] * v[2]));
    }
    return k;
}

// ---- the whole search on the host over n packed pairs: the statement as a loop over the functions above ----------------------------------
// keep (n bytes of 0 / 1) and M (the best hypothesis, RG_MODEL doubles) receive the answer; returns the inlier count, 0 when there is
// no model.  *n_hyp: hypotheses taken; *best_j: -1 when there is no model.
static inline int vp_rg_search_host(const float* pairs, int n, const vp_rg_metric& K, int max_iters, double confidence, uint32_t seed, double M[RG_MODEL], uint8_t* keep,
                                    int* n_hyp, int* best_j)
{
    for (int k = 0; k < RG_MODEL; k++) M[k] = 0.0;
    for (int i = 0; i < n; i++) keep[i] = 0;
    *n_hyp = 0;
    *best_j = -1;
    if (n < 3) return 0;
    int32_t need[RS_MAX_ROUNDS];
    const int rounds = vp_rs_stop_table(n, VP_MODEL_AFFINE, confidence, max_iters, need);
    int best = -1, bj = -1;
    double T[RG_MODEL];
    int32_t s[4];
    for (int r = 0; r < rounds; r++) {
        const int end = (r + 1) * RS_ROUND < max_iters ? (r + 1) * RS_ROUND : max_iters;
        for (int j = r * RS_ROUND; j < end; j++) {
            if (!vp_rg_hypothesis(pairs, pairs + 4, 8, n, seed, (uint32_t)j, s, T)) continue;
            int c = 0;
            for (int i = 0; i < n; i++) c += vp_rg_inlier_packed(T, K, pairs, i);
            if (c > best) {
                best = c;
                bj = j;
                for (int k = 0; k < RG_MODEL; k++) M[k] = T[k];
            }
        }
        *n_hyp = end;
        if (best >= need[r]) break;
    }
    if (best < 3) {
        for (int k = 0; k < RG_MODEL; k++) M[k] = 0.0;
        return 0;
    }
    *best_j = bj;
    int c = 0;
    for (int i = 0; i < n; i++) {
        keep[i] = vp_rg_inlier_packed(M, K, pairs, i);
        c += keep[i];
    }
    return c;
}

static_assert(VP_RIGID_RESULT == 2 * RG_MOTION + 7 && VP_RIGID_COUNTS == 4, "fit rigid: the result layout of include/vp.h");
static_assert(RG_RUN % RG_THREADS == 0 && RG_THREADS % 64 == 0, "fit rigid: a run is whole passes of whole waves");
static_assert((RG_MAX_PAIRS + RG_STAGE - 1) / RG_STAGE <= 65535, "fit rigid: the chunks fit the grid's y extent");
static_assert(RS_ROUND == RG_THREADS && RS_ROUND <= 256, "fit rigid: the select block has one thread per hypothesis and packs its index into 8 bits of a 64-bit key");
static_assert(RG_HYP_PER_BLOCK % (RG_THREADS / 64) == 0 && RG_HYP_PER_BLOCK * RG_MOTION <= RG_THREADS, "fit rigid: the waves take equal turns; one thread stages one number of the block's motions");
static_assert(RG_STAGE * 32 + RG_HYP_PER_BLOCK * (RG_MOTION * 8 + 4) <= 65536, "fit rigid: the staged pairs and motions fit the LDS a kernel gets without asking");
