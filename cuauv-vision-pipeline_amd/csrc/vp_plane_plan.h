// Robust plane fitting to the 3-D points of an image as this library states it (vp_plane.hip; the statement:
// tests/plane_restate.py): the limits and argument checks, the usable-point test, the hypothesis from three points, the inlier test,
// the stop rule, the refit from the ten sums, the host form of the whole search and the plan of the device form.  The mixer, the
// sampler and the stop table are those of vp_model_plan.h.  Plain C++, a pure function of its arguments; what the kernels share is
// __host__ __device__.  Every double expression here is + - * / sqrt and comparisons in one written order, and the units that
// include this file are compiled without floating-point contraction, so device, host and the Python statement give the same bits.
#pragma once
#include <string.h>
#include "vp_model_plan.h"
#include "vp_ws_frame.h"

#define PL_RUN 1024                  // candidates a compaction block counts and ranks: four passes of its 256 threads
#define PL_STAGE RS_STAGE            // points a scoring block stages in LDS at once (16 bytes each)
#define PL_HYP_PER_BLOCK RS_HYP_PER_BLOCK
#define PL_THREADS RS_THREADS
#define PL_MAX_SIDE 4096
#define PL_MODEL 7                   // doubles kept per hypothesis: the plane's four and the sample's first point
#define PL_SUMS 9                    // the sums of the refit besides the count: u v w uu uv uw vv vw ww, u = p - p0
#define PL_VOID_SIN2 1e-12           // a sample is void unless |e1 x e2|^2 > this |e1|^2 |e2|^2
#define PL_MIN_NZ 1e-6               // ALONG_Z: void unless |n2| is above it
#define PL_REFIT_EPS 1e-12
#define PL_JACOBI_SWEEPS 8

// what the device keeps between the launches of one call
struct vp_pl_state {
    int32_t done;                    // the search has ended: later launches return at once
    int32_t rounds;                  // rounds that counted
    int32_t best_count;              // -1: no valid hypothesis so far
    int32_t best_j;
    int32_t n_usable;                // written by the scan, read by everything after it
    int32_t pad;
    double best[PL_MODEL];
    double sums[PL_SUMS];
};

struct vp_pl_box { int x0, y0, rw, rh; };

struct vp_pl_plan {
    vp_pl_box box;
    int ncand;                       // pixels inside the box: the most points there can be
    int rounds;
    unsigned runs;                   // compaction blocks
    unsigned score_gx, score_gy;     // scoring: hypothesis groups x point chunks (of the most points there can be)
    unsigned finish_grid;
};

// the buffers of a call inside the context's workspace
struct vp_pl_buffers {
    float* pts;                      // ncand float4
    int32_t* run_count; int32_t* run_off;
    double* qcrit;                   // per round: the smallest ratio best / n at which the search stops (vp_pl_stop_ratios)
    int32_t* counts; int32_t* valid; double* models;
    vp_pl_state* state;
};

static inline void vp_pl_declare(vp_ws_frame& W, const vp_pl_plan& P, vp_pl_buffers* B)
{
    W.want(&B->pts, (size_t)P.ncand * 16);
    W.want(&B->run_count, (size_t)P.runs * 4);
    W.want(&B->run_off, (size_t)P.runs * 4);
    W.want(&B->qcrit, (size_t)P.rounds * 8);
    W.want(&B->counts, RS_ROUND * 4);
    W.want(&B->valid, RS_ROUND * 4);
    W.want(&B->models, RS_ROUND * PL_MODEL * 8);
    W.want(&B->state, sizeof(vp_pl_state));
}

// NULL: admitted; else the reason (VP_ERR_INVALID).  What does not depend on pointers.
static inline const char* vp_pl_size_refusal(int w, int h, const int32_t* box)
{
    if (w < 1 || w > PL_MAX_SIDE || h < 1 || h > PL_MAX_SIDE) return "fit plane: the image must be 1 to 4096 pixels wide and high";
    if (box) {
        if (box[2] < 1 || box[3] < 1) return "fit plane: the box is empty";
        if (box[0] < 0 || box[1] < 0 || box[0] > w - box[2] || box[1] > h - box[3]) return "fit plane: the box leaves the image";
    }
    return nullptr;
}

static inline const char* vp_pl_search_refusal(int metric, double threshold, int max_iters, double confidence)
{
    if (metric != VP_PLANE_PERP && metric != VP_PLANE_ALONG_Z) return "fit plane: unknown metric";
    if (!(threshold > 0) || !isfinite(threshold)) return "fit plane: the threshold must be finite and above 0";
    if (max_iters < 1 || max_iters > RS_MAX_ITERS) return "fit plane: max_iters must be 1 to 65536";
    if (!(confidence > 0 && confidence < 1)) return "fit plane: the confidence must be above 0 and below 1";
    return nullptr;
}

static inline void vp_pl_make_plan(int w, int h, const int32_t* box, int max_iters, vp_pl_plan* P)
{
    P->box = box ? vp_pl_box{box[0], box[1], box[2], box[3]} : vp_pl_box{0, 0, w, h};
    P->ncand = P->box.rw * P->box.rh;
    P->rounds = vp_rs_round_count(max_iters);
    P->runs = (unsigned)((P->ncand + PL_RUN - 1) / PL_RUN);
    P->score_gx = RS_ROUND / PL_HYP_PER_BLOCK;
    P->score_gy = (unsigned)((P->ncand + PL_STAGE - 1) / PL_STAGE);
    P->finish_grid = (unsigned)((P->ncand + PL_THREADS - 1) / PL_THREADS);
}

// ---- points ----------------------------------------------------------------------------------------------------------------------------
// finite, and not the three zeros with which the library writes "unknown"
VP_RS_HD static inline bool vp_pl_usable(float x, float y, float z)
{
    const bool fin = x - x == 0.0f && y - y == 0.0f && z - z == 0.0f;
    return fin && !(x == 0.0f && y == 0.0f && z == 0.0f);
}

VP_RS_HD static inline double vp_pl_sqrt(double v)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __dsqrt_rn(v);
#else
    return sqrt(v);
#endif
}

// ---- the plane through three points, oriented towards the camera (d > 0); 1 valid, 0 void ---------------------------------------------
VP_RS_HD static inline int vp_pl_plane_from(const double* p0, const double* p1, const double* p2, int metric, double* P)
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
    const double len = vp_pl_sqrt(l2);
    double n0 = c0 / len, n1 = c1 / len, n2 = c2 / len;
    double d = -(((n0 * p0[0]) + (n1 * p0[1])) + (n2 * p0[2]));
    if (d < 0) { n0 = -n0; n1 = -n1; n2 = -n2; d = -d; }
    if (d == 0 || !(vp_rs_finite(n0) && vp_rs_finite(n1) && vp_rs_finite(n2) && vp_rs_finite(d))) return 0;
    if (metric == VP_PLANE_ALONG_Z && !(vp_rs_abs(n2) > PL_MIN_NZ)) return 0;
    P[0] = n0; P[1] = n1; P[2] = n2; P[3] = d;
    return 1;
}

// hypothesis j over n packed points (x, y, z, pixel index; 4 floats each): its sample -> s[0 .. 3), its PL_MODEL doubles -> M (zeros
// when void)
VP_RS_HD static inline int vp_pl_hypothesis(const float* pts, int n, int metric, uint32_t seed, uint32_t j, int32_t s[4], double M[PL_MODEL])
{
    for (int k = 0; k < PL_MODEL; k++) M[k] = 0.0;
    if (!vp_rs_sample(n, 3, seed, j, s)) return 0;
    double p[3][3];
    for (int k = 0; k < 3; k++)
        for (int c = 0; c < 3; c++) p[k][c] = (double)pts[(size_t)s[k] * 4 + c];
    double P[4];
    if (!vp_pl_plane_from(p[0], p[1], p[2], metric, P)) return 0;
    for (int k = 0; k < 4; k++) M[k] = P[k];
    for (int c = 0; c < 3; c++) M[4 + c] = p[0][c];
    return 1;
}

// the bound of e e for plane P under the metric: t2, or t2 n2 n2 when the residual is taken along the third axis
VP_RS_HD static inline double vp_pl_limit(const double* P, int metric, double t2) { return metric == VP_PLANE_ALONG_Z ? t2 * (P[2] * P[2]) : t2; }

VP_RS_HD static inline bool vp_pl_inlier(const double* P, double lim, double x, double y, double z)
{
    const double e = (((P[0] * x) + (P[1] * y)) + (P[2] * z)) + P[3];
    return e * e <= lim;
}

// ---- the stop rule ---------------------------------------------------------------------------------------------------------------------
// The statement stops after round r once the best count has reached need[r], the smallest c in 3 .. n (by bisection) with
// num_iters(confidence, 1 - c / n) <= r RS_ROUND.  The device learns n only when it has compacted the points, and num_iters is libm,
// which the host alone calls.  So the host inverts the libm part: q[r - 1] is the smallest double q in [0, 1] with
// num_iters(confidence, 1 - q) <= r RS_ROUND (bisection over the bit patterns; the number falls as q grows and is 0 at q = 1), and the
// device, which has n and the best count c, tests (double)c / (double)n >= q[r - 1]: the same division the bisection over c makes,
// so the answer is that of need[r] for the true n.
static inline int vp_pl_stop_ratios(double confidence, int max_iters, double* q)
{
    const int rounds = vp_rs_round_count(max_iters);
    for (int r = 1; r <= rounds; r++) {
        uint64_t lo = 0, hi = 0x3ff0000000000000ull;      // 0.0 and 1.0: non-negative doubles order as their bits do
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            double v;
            memcpy(&v, &mid, 8);
            if (vp_rs_num_iters(confidence, 1.0 - v, 3, max_iters) <= r * RS_ROUND) hi = mid;
            else lo = mid + 1;
        }
        memcpy(&q[r - 1], &lo, 8);
    }
    return rounds;
}

VP_RS_HD static inline bool vp_pl_stop(int best, int n, double q) { return best >= 3 && (double)best / (double)n >= q; }

// ---- the refit from the count and the nine sums about p0 -> result[12]: plane 4, best hypothesis 4, centroid 3, rms --------------------
static inline void vp_pl_jacobi3(double A[3][3], double V[3][3])
{
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) V[r][c] = r == c ? 1.0 : 0.0;
    const int pq[3][2] = {{0, 1}, {0, 2}, {1, 2}};
    for (int sweep = 0; sweep < PL_JACOBI_SWEEPS; sweep++)
        for (int i = 0; i < 3; i++) {
            const int p = pq[i][0], q = pq[i][1], r = 3 - p - q;
            const double apq = A[p][q];
            if (apq == 0.0 || !vp_rs_finite(apq)) continue;
            const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
            double t = 1.0 / (vp_rs_abs(theta) + sqrt((theta * theta) + 1.0));
            if (theta < 0) t = -t;
            const double c = 1.0 / sqrt((t * t) + 1.0), s = t * c;
            const double app = A[p][p], aqq = A[q][q], arp = A[r][p], arq = A[r][q];
            A[p][p] = app - (t * apq);
            A[q][q] = aqq + (t * apq);
            A[p][q] = A[q][p] = 0.0;
            A[r][p] = A[p][r] = (c * arp) - (s * arq);
            A[r][q] = A[q][r] = (s * arp) + (c * arq);
            for (int k = 0; k < 3; k++) {
                const double vkp = V[k][p], vkq = V[k][q];
                V[k][p] = (c * vkp) - (s * vkq);
                V[k][q] = (s * vkp) + (c * vkq);
            }
        }
}

// best: the best hypothesis, or NULL for the refit alone.  Returns 1; 0 (zeros) when there are fewer than three points, or when the
// refit is degenerate and there is no hypothesis to fall back to.
static inline int vp_pl_refit_close(int k, const double* S, const double* p0, int metric, const double* best, double* result)
{
    for (int i = 0; i < VP_PLANE_RESULT; i++) result[i] = 0.0;
    if (k < 3) return 0;
    const double kk = (double)k;
    const double mu[3] = {S[0] / kk, S[1] / kk, S[2] / kk};
    const double cen[3] = {p0[0] + mu[0], p0[1] + mu[1], p0[2] + mu[2]};
    const double Cuu = S[3] - ((S[0] * S[0]) / kk), Cuv = S[4] - ((S[0] * S[1]) / kk), Cuw = S[5] - ((S[0] * S[2]) / kk);
    const double Cvv = S[6] - ((S[1] * S[1]) / kk), Cvw = S[7] - ((S[1] * S[2]) / kk), Cww = S[8] - ((S[2] * S[2]) / kk);
    double plane[4] = {0, 0, 0, 0}, rms = 0.0;
    bool ok = false;
    if (metric == VP_PLANE_PERP) {
        double A[3][3] = {{Cuu, Cuv, Cuw}, {Cuv, Cvv, Cvw}, {Cuw, Cvw, Cww}}, V[3][3];
        vp_pl_jacobi3(A, V);
        const double lam[3] = {A[0][0], A[1][1], A[2][2]};
        int lo = 0, hi = 0;
        for (int i = 1; i < 3; i++) if (lam[i] < lam[lo]) lo = i;
        for (int i = 1; i < 3; i++) if (lam[i] > lam[hi]) hi = i;
        const int mid = lo != hi ? 3 - lo - hi : -1;
        if (mid >= 0 && lam[mid] > PL_REFIT_EPS * lam[hi]) {      // else the inliers lie on a line (or are one point)
            double n[3] = {V[0][lo], V[1][lo], V[2][lo]};
            const double len = sqrt(((n[0] * n[0]) + (n[1] * n[1])) + (n[2] * n[2]));
            for (int c = 0; c < 3; c++) n[c] = n[c] / len;
            plane[0] = n[0]; plane[1] = n[1]; plane[2] = n[2];
            plane[3] = -(((n[0] * cen[0]) + (n[1] * cen[1])) + (n[2] * cen[2]));
            rms = sqrt((lam[lo] > 0 ? lam[lo] : 0.0) / kk);
            ok = true;
        }
    } else {
        const double det = (Cuu * Cvv) - (Cuv * Cuv);
        if (det > PL_REFIT_EPS * (Cuu * Cvv)) {
            const double a = ((Cuw * Cvv) - (Cvw * Cuv)) / det, b = ((Cvw * Cuu) - (Cuw * Cuv)) / det;
            const double len = sqrt(((a * a) + (b * b)) + 1.0);
            plane[0] = a / len; plane[1] = b / len; plane[2] = -1.0 / len;
            plane[3] = (cen[2] - ((a * cen[0]) + (b * cen[1]))) / len;
            const double ss = ((Cww - (2.0 * ((a * Cuw) + (b * Cvw)))) + (((a * a) * Cuu) + ((b * b) * Cvv))) + ((2.0 * (a * b)) * Cuv);
            rms = sqrt((ss > 0 ? ss : 0.0) / kk);
            ok = true;
        }
    }
    if (ok && plane[3] < 0)
        for (int c = 0; c < 4; c++) plane[c] = -plane[c];
    ok = ok && vp_rs_finite(plane[0]) && vp_rs_finite(plane[1]) && vp_rs_finite(plane[2]) && vp_rs_finite(plane[3]) && vp_rs_finite(rms) && plane[3] > 0;
    if (!ok) {
        if (!best) return 0;
        // the best hypothesis stands; its residual from the same sums: e_i = n.u_i + e0 (ALONG_Z: divided by |n2|)
        const double* n = best;
        const double e0 = (((best[0] * p0[0]) + (best[1] * p0[1])) + (best[2] * p0[2])) + best[3];
        const double q = ((((n[0] * n[0]) * S[3]) + ((n[1] * n[1]) * S[6])) + ((n[2] * n[2]) * S[8])) +
                         (2.0 * ((((n[0] * n[1]) * S[4]) + ((n[0] * n[2]) * S[5])) + ((n[1] * n[2]) * S[7])));
        double ss = (q + ((2.0 * e0) * (((n[0] * S[0]) + (n[1] * S[1])) + (n[2] * S[2])))) + ((kk * e0) * e0);
        if (metric == VP_PLANE_ALONG_Z) ss = ss / (n[2] * n[2]);
        rms = sqrt((ss > 0 ? ss : 0.0) / kk);
        if (!vp_rs_finite(rms)) rms = 0.0;
        for (int c = 0; c < 4; c++) plane[c] = best[c];
    }
    for (int c = 0; c < 4; c++) result[c] = plane[c];
    if (best)
        for (int c = 0; c < 4; c++) result[4 + c] = best[c];
    for (int c = 0; c < 3; c++) result[8 + c] = cen[c];
    result[11] = rms;
    return 1;
}

// the count and the nine sums over the packed points whose keep byte is not 0 (keep NULL: all), in index order
static inline int vp_pl_sums_host(const float* pts, int n, const uint8_t* keep, const double* p0, double* S)
{
    int k = 0;
    for (int i = 0; i < PL_SUMS; i++) S[i] = 0.0;
    for (int i = 0; i < n; i++) {
        if (keep && !keep[i]) continue;
        const double u = (double)pts[(size_t)i * 4] - p0[0], v = (double)pts[(size_t)i * 4 + 1] - p0[1], w = (double)pts[(size_t)i * 4 + 2] - p0[2];
        k++;
        S[0] = S[0] + u; S[1] = S[1] + v; S[2] = S[2] + w;
        S[3] = S[3] + u * u; S[4] = S[4] + u * v; S[5] = S[5] + u * w;
        S[6] = S[6] + v * v; S[7] = S[7] + v * w; S[8] = S[8] + w * w;
    }
    return k;
}

// ---- the whole search on the host over n packed points: the statement as a loop over the functions above -------------------------------
// keep (n bytes of 0 / 1) and M (the best hypothesis, PL_MODEL doubles) receive the answer; returns the inlier count, 0 when there is
// no model.  *n_hyp: hypotheses taken; *best_j: -1 when there is no model.
static inline int vp_pl_search_host(const float* pts, int n, int metric, double t2, int max_iters, double confidence, uint32_t seed, double M[PL_MODEL],
                                    uint8_t* keep, int* n_hyp, int* best_j)
{
    for (int k = 0; k < PL_MODEL; k++) M[k] = 0.0;
    for (int i = 0; i < n; i++) keep[i] = 0;
    *n_hyp = 0;
    *best_j = -1;
    if (n < 3) return 0;
    int32_t need[RS_MAX_ROUNDS];
    const int rounds = vp_rs_stop_table(n, VP_MODEL_AFFINE, confidence, max_iters, need);
    int best = -1, bj = -1;
    double T[PL_MODEL];
    int32_t s[4];
    for (int r = 0; r < rounds; r++) {
        const int end = (r + 1) * RS_ROUND < max_iters ? (r + 1) * RS_ROUND : max_iters;
        for (int j = r * RS_ROUND; j < end; j++) {
            if (!vp_pl_hypothesis(pts, n, metric, seed, (uint32_t)j, s, T)) continue;
            const double lim = vp_pl_limit(T, metric, t2);
            int c = 0;
            for (int i = 0; i < n; i++) c += vp_pl_inlier(T, lim, (double)pts[(size_t)i * 4], (double)pts[(size_t)i * 4 + 1], (double)pts[(size_t)i * 4 + 2]);
            if (c > best) {
                best = c;
                bj = j;
                for (int k = 0; k < PL_MODEL; k++) M[k] = T[k];
            }
        }
        *n_hyp = end;
        if (best >= need[r]) break;
    }
    if (best < 3) {
        for (int k = 0; k < PL_MODEL; k++) M[k] = 0.0;
        return 0;
    }
    *best_j = bj;
    const double lim = vp_pl_limit(M, metric, t2);
    int c = 0;
    for (int i = 0; i < n; i++) {
        keep[i] = vp_pl_inlier(M, lim, (double)pts[(size_t)i * 4], (double)pts[(size_t)i * 4 + 1], (double)pts[(size_t)i * 4 + 2]);
        c += keep[i];
    }
    return c;
}

static_assert(VP_PLANE_RESULT == 12 && VP_PLANE_COUNTS == 4, "fit plane: the result layout of include/vp.h");
static_assert(PL_RUN % PL_THREADS == 0 && PL_THREADS % 64 == 0 && PL_RUN / 64 <= 64, "fit plane: a run is whole passes of whole waves, its wave counts fit one wave's scan");
static_assert((long long)PL_MAX_SIDE * PL_MAX_SIDE < (1ll << 31), "fit plane: a pixel index is an int");
static_assert(((long long)PL_MAX_SIDE * PL_MAX_SIDE + PL_STAGE - 1) / PL_STAGE <= 65535, "fit plane: the chunks fit the grid's y extent");
static_assert(RS_ROUND == PL_THREADS && RS_ROUND <= 256, "fit plane: the select block has one thread per hypothesis and packs its index into 8 bits of a 64-bit key");
static_assert(PL_STAGE * 16 <= 65536, "fit plane: the staged points fit the LDS a kernel gets without asking");
