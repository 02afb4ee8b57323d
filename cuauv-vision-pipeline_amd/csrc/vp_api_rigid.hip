// C ABI of libvp.so, robust rigid 3-D motion between paired 3-D points (kernels: vp_rigid.hip; checks, pair of a track, hypothesis,
// inlier tests, refit, host form and plan: vp_rigid_plan.h), on host and device arrays, on tracks into two images of points, and the
// same statement as plain scalar C++.
#include "vp_api_util.h"
#include "vp_rigid_plan.h"

int vpk_rg_run(vp_ctx* ctx, const vp_rg_plan& P, const vp_rg_buffers& B, const float* d_src, const float* d_dst, const vp_rg_tracks* tracks, const vp_rg_metric& K,
               int max_iters, u32 seed, uint8_t* d_inl);

struct rigid_search { int metric; double threshold, focal_px, baseline; int max_iters; double confidence; uint32_t seed; };

// everything the array entries refuse, from the arguments alone
static const char* rigid_check(const float* src, const float* dst, int n, const rigid_search& A, const uint8_t* inliers, const double* result, const int32_t* counts)
{
    if (!src || !dst || !result || !counts) return "fit rigid: a pointer is missing";
    if (const char* why = vp_rg_count_refusal(n)) return why;
    if ((uintptr_t)src % 4 || (uintptr_t)dst % 4) return "fit rigid: the points are not aligned to their element size";
    if (const char* why = vp_rg_search_refusal(A.metric, A.threshold, A.focal_px, A.baseline, A.max_iters, A.confidence)) return why;
    if (inliers && (dev_overlap(inliers, (size_t)n, src, (size_t)n * 12) || dev_overlap(inliers, (size_t)n, dst, (size_t)n * 12)))
        return "fit rigid: the inlier bytes overlap the points";
    return nullptr;
}

// everything the track entries refuse; inliers_on_host: the inlier bytes are host memory, as prev_pts always is
static const char* tracks_check(const float* xyz0, size_t stride0, const float* xyz1, size_t stride1, int w, int h, const float* prev, const void* rows, int n,
                                const rigid_search& A, const uint8_t* inliers, bool inliers_on_host, const double* result, const int32_t* counts)
{
    if (!xyz0 || !xyz1 || !prev || !rows || !result || !counts) return "fit rigid: a pointer is missing";
    if (const char* why = vp_rg_count_refusal(n)) return why;
    if (const char* why = vp_rg_size_refusal(w, h)) return why;
    if (stride0 < (size_t)w * 12 || stride1 < (size_t)w * 12) return "fit rigid: a stride is below the row";
    if (stride0 % 4 || stride1 % 4) return "fit rigid: a stride is no multiple of 4";
    if ((uintptr_t)xyz0 % 4 || (uintptr_t)xyz1 % 4 || (uintptr_t)prev % 4 || (uintptr_t)rows % 4) return "fit rigid: an input is not aligned to its element size";
    if (const char* why = vp_rg_search_refusal(A.metric, A.threshold, A.focal_px, A.baseline, A.max_iters, A.confidence)) return why;
    if (inliers) {
        const size_t ib = (size_t)n;
        if (dev_overlap(inliers, ib, xyz0, strided_bytes(stride0, (size_t)w * 12, h)) || dev_overlap(inliers, ib, xyz1, strided_bytes(stride1, (size_t)w * 12, h)))
            return "fit rigid: the inlier bytes overlap an image";
        if (dev_overlap(inliers, ib, rows, (size_t)n * 16)) return "fit rigid: the inlier bytes overlap the tracks";
        if (inliers_on_host && dev_overlap(inliers, ib, prev, (size_t)n * 8)) return "fit rigid: the inlier bytes overlap prev_pts";
    }
    return nullptr;
}

static void rigid_answer(bool found, int k, const double* S, const double* M, int n_usable, int taken, int best_j, double* result, int32_t* counts)
{
    for (int i = 0; i < VP_RIGID_RESULT; i++) result[i] = 0.0;
    if (found) vp_rg_refit_close(k, S, M + 12, M + 15, M, result);
    counts[0] = n_usable;
    counts[1] = found ? k : 0;
    counts[2] = taken;
    counts[3] = found ? best_j : -1;
}

// device inputs in, the device inlier bytes (nullable) out, copied to h_inl (nullable) as well; enqueues every launch and
// synchronises once
static int rigid_run(vp_ctx* ctx, const vp_rg_plan& P, const vp_rg_buffers& B, const float* d_src, const float* d_dst, const vp_rg_tracks* tracks, const rigid_search& A,
                     uint8_t* d_inl, uint8_t* h_inl, double* result, int32_t* counts)
{
    const size_t qbytes = (size_t)P.rounds * 8;
    int slot = -1;
    uint8_t* hq = vp_ring_take(ctx, qbytes, &slot);
    if (!hq) return vp_fail(ctx, VP_ERR_NOMEM, "pinned staging");
    vp_pl_stop_ratios(A.confidence, A.max_iters, reinterpret_cast<double*>(hq));
    int rc = h2d(ctx, B.qcrit, hq, qbytes);
    if (rc == VP_OK) rc = vpk_rg_run(ctx, P, B, d_src, d_dst, tracks, vp_rg_make_metric(A.metric, A.threshold, A.focal_px, A.baseline), A.max_iters, A.seed, d_inl);
    vp_ring_done(ctx, slot);
    VP_TRY(rc);
    vp_rg_state* st = (vp_rg_state*)vp_hstage(ctx, sizeof(vp_rg_state));
    if (!st) return vp_fail(ctx, VP_ERR_NOMEM, "pinned staging");
    VP_TRY(d2h(ctx, st, B.state, sizeof(vp_rg_state)));
    if (h_inl) VP_TRY(d2h(ctx, h_inl, d_inl, (size_t)P.n));
    VP_TRY(vp_synchronize(ctx));
    const int taken = st->rounds * RS_ROUND < A.max_iters ? st->rounds * RS_ROUND : A.max_iters;
    rigid_answer(st->best_count >= 3, st->best_count, st->sums, st->best, st->n_usable, taken, st->best_j, result, counts);
    return VP_OK;
}

// the host form over packed pairs whose original indices are `index`
static void rigid_host(const std::vector<float>& pairs, const std::vector<int32_t>& index, int n_given, const rigid_search& A, uint8_t* inliers, double* result,
                       int32_t* counts)
{
    const int n = (int)index.size();
    std::vector<uint8_t> keep((size_t)n + 1);
    double M[RG_MODEL], S[RG_SUMS];
    int taken = 0, best_j = -1;
    const vp_rg_metric K = vp_rg_make_metric(A.metric, A.threshold, A.focal_px, A.baseline);
    const int c = vp_rg_search_host(pairs.data(), n, K, A.max_iters, A.confidence, A.seed, M, keep.data(), &taken, &best_j);
    const int k = c >= 3 ? vp_rg_sums_host(pairs.data(), pairs.data() + 4, 8, n, keep.data(), M + 12, M + 15, S) : 0;
    rigid_answer(c >= 3, k, S, M, n, taken, best_j, result, counts);
    if (inliers) {
        memset(inliers, 0, (size_t)n_given);
        for (int i = 0; i < n; i++)
            if (keep[i]) inliers[index[i]] = 1;
    }
}

static void rigid_pack(const float* p, const float* q, int i, std::vector<float>* pairs, std::vector<int32_t>* index)
{
    float bits;
    const int32_t at = i;
    memcpy(&bits, &at, 4);
    pairs->insert(pairs->end(), {p[0], p[1], p[2], bits, q[0], q[1], q[2], 0.0f});
    index->push_back(i);
}

extern "C" {

int vp_fit_rigid_plan(int n, size_t* ws_bytes, int32_t* geometry)
{
    if (!ws_bytes || !geometry) return vp_fail(nullptr, VP_ERR_INVALID, "fit rigid: a pointer is missing");
    if (const char* why = vp_rg_count_refusal(n)) return vp_fail(nullptr, VP_ERR_INVALID, why);
    vp_rg_plan P;
    vp_rg_make_plan(n, RS_MAX_ITERS, &P);
    vp_rg_buffers B;
    vp_ws_frame W;
    vp_rg_declare(W, P, &B);
    *ws_bytes = W.bytes();
    geometry[0] = RG_RUN;
    geometry[1] = RG_STAGE;
    geometry[2] = RG_HYP_PER_BLOCK;
    geometry[3] = RG_THREADS;
    geometry[4] = RS_ROUND;
    geometry[5] = P.n;
    geometry[6] = (int32_t)P.runs;
    geometry[7] = (int32_t)P.score_gy;
    return VP_OK;
}

int vp_fit_rigid_dev(vp_ctx* ctx, const float* src_dev, const float* dst_dev, int n, int metric, double threshold, double focal_px, double baseline, int max_iters,
                     double confidence, uint32_t seed, uint8_t* inliers_dev, double* result, int32_t* counts)
{
    const rigid_search A = {metric, threshold, focal_px, baseline, max_iters, confidence, seed};
    if (const char* why = rigid_check(src_dev, dst_dev, n, A, inliers_dev, result, counts)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    vp_rg_plan P;
    vp_rg_make_plan(n, max_iters, &P);
    vp_rg_buffers B;
    vp_ws_frame W;
    vp_rg_declare(W, P, &B);
    VP_TRY(vp_ws_commit(ctx, W, "vp_fit_rigid_dev"));
    return rigid_run(ctx, P, B, src_dev, dst_dev, nullptr, A, inliers_dev, nullptr, result, counts);
}

int vp_fit_rigid_f32(vp_ctx* ctx, const float* src, const float* dst, int n, int metric, double threshold, double focal_px, double baseline, int max_iters,
                     double confidence, uint32_t seed, uint8_t* inliers, double* result, int32_t* counts)
{
    const rigid_search A = {metric, threshold, focal_px, baseline, max_iters, confidence, seed};
    if (const char* why = rigid_check(src, dst, n, A, inliers, result, counts)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    vp_rg_plan P;
    vp_rg_make_plan(n, max_iters, &P);
    vp_rg_buffers B;
    vp_ws_frame W;
    vp_rg_declare(W, P, &B);
    float* d_src; W.want(&d_src, (size_t)n * 12);
    float* d_dst; W.want(&d_dst, (size_t)n * 12);
    uint8_t* d_inl = nullptr; if (inliers) W.want(&d_inl, (size_t)n);
    VP_TRY(vp_ws_commit(ctx, W, "vp_fit_rigid_f32"));
    VP_TRY(h2d(ctx, d_src, src, (size_t)n * 12));
    VP_TRY(h2d(ctx, d_dst, dst, (size_t)n * 12));
    return rigid_run(ctx, P, B, d_src, d_dst, nullptr, A, d_inl, inliers, result, counts);
}

int vp_fit_rigid_host(const float* src, const float* dst, int n, int metric, double threshold, double focal_px, double baseline, int max_iters, double confidence,
                      uint32_t seed, uint8_t* inliers, double* result, int32_t* counts)
{
    const rigid_search A = {metric, threshold, focal_px, baseline, max_iters, confidence, seed};
    if (const char* why = rigid_check(src, dst, n, A, inliers, result, counts)) return vp_fail(nullptr, VP_ERR_INVALID, why);
    std::vector<float> pairs;
    std::vector<int32_t> index;
    for (int i = 0; i < n; i++) {
        const float* p = src + (size_t)i * 3;
        const float* q = dst + (size_t)i * 3;
        if (vp_pl_usable(p[0], p[1], p[2]) && vp_pl_usable(q[0], q[1], q[2])) rigid_pack(p, q, i, &pairs, &index);
    }
    rigid_host(pairs, index, n, A, inliers, result, counts);
    return VP_OK;
}

int vp_fit_rigid_tracks_dev(vp_ctx* ctx, const float* xyz_prev_dev, size_t xyz_prev_stride, const float* xyz_cur_dev, size_t xyz_cur_stride, int w, int h,
                            const float* prev_pts_host, const void* tracks_dev, int n, int metric, double threshold, double focal_px, double baseline, int max_iters,
                            double confidence, uint32_t seed, uint8_t* inliers_dev, double* result, int32_t* counts)
{
    const rigid_search A = {metric, threshold, focal_px, baseline, max_iters, confidence, seed};
    if (const char* why = tracks_check(xyz_prev_dev, xyz_prev_stride, xyz_cur_dev, xyz_cur_stride, w, h, prev_pts_host, tracks_dev, n, A, inliers_dev, false, result, counts))
        return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    vp_rg_plan P;
    vp_rg_make_plan(n, max_iters, &P);
    vp_rg_buffers B;
    vp_ws_frame W;
    vp_rg_declare(W, P, &B);
    float* d_prev; W.want(&d_prev, (size_t)n * 8);
    VP_TRY(vp_ws_commit(ctx, W, "vp_fit_rigid_tracks_dev"));
    VP_TRY(h2d(ctx, d_prev, prev_pts_host, (size_t)n * 8));
    const vp_rg_tracks T = {xyz_prev_dev, xyz_prev_stride, xyz_cur_dev, xyz_cur_stride, w, h, d_prev, static_cast<const uint32_t*>(tracks_dev)};
    return rigid_run(ctx, P, B, nullptr, nullptr, &T, A, inliers_dev, nullptr, result, counts);
}

int vp_fit_rigid_tracks_f32(vp_ctx* ctx, const float* xyz_prev, const float* xyz_cur, int w, int h, const float* prev_pts, const void* tracks, int n, int metric,
                            double threshold, double focal_px, double baseline, int max_iters, double confidence, uint32_t seed, uint8_t* inliers, double* result,
                            int32_t* counts)
{
    const rigid_search A = {metric, threshold, focal_px, baseline, max_iters, confidence, seed};
    const size_t row = w > 0 ? (size_t)w * 12 : 0;
    if (const char* why = tracks_check(xyz_prev, row, xyz_cur, row, w, h, prev_pts, tracks, n, A, inliers, true, result, counts)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    vp_rg_plan P;
    vp_rg_make_plan(n, max_iters, &P);
    vp_rg_buffers B;
    vp_ws_frame W;
    vp_rg_declare(W, P, &B);
    float* d_xyz0; W.want(&d_xyz0, row * h);
    float* d_xyz1; W.want(&d_xyz1, row * h);
    float* d_prev; W.want(&d_prev, (size_t)n * 8);
    uint32_t* d_rows; W.want(&d_rows, (size_t)n * 16);
    uint8_t* d_inl = nullptr; if (inliers) W.want(&d_inl, (size_t)n);
    VP_TRY(vp_ws_commit(ctx, W, "vp_fit_rigid_tracks_f32"));
    VP_TRY(h2d(ctx, d_xyz0, xyz_prev, row * h));
    VP_TRY(h2d(ctx, d_xyz1, xyz_cur, row * h));
    VP_TRY(h2d(ctx, d_prev, prev_pts, (size_t)n * 8));
    VP_TRY(h2d(ctx, d_rows, tracks, (size_t)n * 16));
    const vp_rg_tracks T = {d_xyz0, row, d_xyz1, row, w, h, d_prev, d_rows};
    return rigid_run(ctx, P, B, nullptr, nullptr, &T, A, d_inl, inliers, result, counts);
}

int vp_fit_rigid_tracks_host(const float* xyz_prev, size_t xyz_prev_stride, const float* xyz_cur, size_t xyz_cur_stride, int w, int h, const float* prev_pts,
                             const void* tracks, int n, int metric, double threshold, double focal_px, double baseline, int max_iters, double confidence, uint32_t seed,
                             uint8_t* inliers, double* result, int32_t* counts)
{
    const rigid_search A = {metric, threshold, focal_px, baseline, max_iters, confidence, seed};
    if (const char* why = tracks_check(xyz_prev, xyz_prev_stride, xyz_cur, xyz_cur_stride, w, h, prev_pts, tracks, n, A, inliers, true, result, counts))
        return vp_fail(nullptr, VP_ERR_INVALID, why);
    const vp_rg_tracks T = {xyz_prev, xyz_prev_stride, xyz_cur, xyz_cur_stride, w, h, prev_pts, static_cast<const uint32_t*>(tracks)};
    std::vector<float> pairs;
    std::vector<int32_t> index;
    for (int i = 0; i < n; i++) {
        float p[3], q[3];
        if (vp_rg_track_pair(T, i, p, q)) rigid_pack(p, q, i, &pairs, &index);
    }
    rigid_host(pairs, index, n, A, inliers, result, counts);
    return VP_OK;
}

int vp_rigid_hypothesis(const float* src3, const float* dst3, int n, uint32_t seed, int j, int32_t* sample3, double* motion12)
{
    if (!src3 || !dst3 || !sample3 || !motion12) return vp_fail(nullptr, VP_ERR_INVALID, "fit rigid: a pointer is missing");
    if (n < 0 || n > RG_MAX_PAIRS) return vp_fail(nullptr, VP_ERR_INVALID, "fit rigid: at most 1048576 pairs");
    if (j < 0 || j >= RS_MAX_ITERS) return vp_fail(nullptr, VP_ERR_INVALID, "fit rigid: the hypothesis index must be 0 to 65535");
    int32_t s[4];
    double M[RG_MODEL];
    const int ok = vp_rg_hypothesis(src3, dst3, 3, n, seed, (uint32_t)j, s, M);
    for (int k = 0; k < 3; k++) sample3[k] = s[k];
    for (int k = 0; k < RG_MOTION; k++) motion12[k] = M[k];
    return ok;
}

int vp_rigid_refit(const float* src3, const float* dst3, int n, const uint8_t* keep /*nullable*/, double* result)
{
    if (!src3 || !dst3 || !result) return vp_fail(nullptr, VP_ERR_INVALID, "fit rigid: a pointer is missing");
    if (n < 0 || n > RG_MAX_PAIRS) return vp_fail(nullptr, VP_ERR_INVALID, "fit rigid: at most 1048576 pairs");
    for (int i = 0; i < VP_RIGID_RESULT; i++) result[i] = 0.0;
    int first = 0;
    while (first < n && keep && !keep[first]) first++;
    if (first >= n) return 0;
    double p0[3], q0[3], S[RG_SUMS];
    for (int c = 0; c < 3; c++) { p0[c] = (double)src3[(size_t)first * 3 + c]; q0[c] = (double)dst3[(size_t)first * 3 + c]; }
    const int k = vp_rg_sums_host(src3, dst3, 3, n, keep, p0, q0, S);
    return vp_rg_refit_close(k, S, p0, q0, nullptr, result);
}

}  // extern "C"
