// C ABI of libvp.so, robust motion estimation from point pairs: cv2.findHomography, estimateAffine2D and estimateAffinePartial2D
// (kernels: vp_model.hip; checks, sampler, solvers, stop table, refit, host form and plan: vp_model_plan.h).
#include "vp_api_util.h"
#include "vp_model_plan.h"

int vpk_rs_pack(vp_ctx* ctx, const float* d_src, const float* d_dst, int n, float* d_pts);
int vpk_rs_search(vp_ctx* ctx, const vp_rs_plan& P, uint8_t* d_ws, int n, int model, double t2, int max_iters, u32 seed);

static const char* rs_check(const void* src, const void* dst, int n, int model, double threshold, int max_iters, double confidence, const double* model_out,
                            const int* n_inliers, const int* n_hypotheses)
{
    if (!src || !dst || !model_out || !n_inliers || !n_hypotheses) return "motion model: a pointer is missing";
    return vp_rs_refusal(n, model, threshold, max_iters, confidence);
}

// the search over the packed points at the head of d_ws (already enqueued there), the stop table, the answer; synchronises once.
// h_pts: the packed points on the host for the refit, or NULL to fetch them with the mask.
static int rs_run(vp_ctx* ctx, const vp_rs_plan& P, uint8_t* d_ws, const float* h_pts, int n, int model, double threshold, int max_iters, double confidence, u32 seed,
                  double* model_out, uint8_t* inliers_host, int* n_inliers, int* n_hypotheses)
{
    const size_t nbytes = (size_t)P.rounds * 4;
    int slot = -1;
    uint8_t* hn = vp_ring_take(ctx, nbytes, &slot);
    if (!hn) return vp_fail(ctx, VP_ERR_NOMEM, "pinned staging");
    vp_rs_stop_table(n, model, confidence, max_iters, reinterpret_cast<int32_t*>(hn));
    int rc = h2d(ctx, d_ws + P.off_need, hn, nbytes);
    if (rc == VP_OK) rc = vpk_rs_search(ctx, P, d_ws, n, model, threshold * threshold, max_iters, seed);
    vp_ring_done(ctx, slot);
    VP_TRY(rc);
    const size_t off_mask = vp_align(sizeof(vp_rs_state)), off_pts = off_mask + vp_align((size_t)n);
    uint8_t* hs = (uint8_t*)vp_hstage(ctx, off_pts + (h_pts ? 0 : (size_t)n * 16));
    if (!hs) return vp_fail(ctx, VP_ERR_NOMEM, "pinned staging");
    VP_TRY(d2h(ctx, hs, d_ws + P.off_state, sizeof(vp_rs_state)));
    VP_TRY(d2h(ctx, hs + off_mask, d_ws + P.off_mask, (size_t)n));
    if (!h_pts) VP_TRY(d2h(ctx, hs + off_pts, d_ws, (size_t)n * 16));
    VP_TRY(vp_synchronize(ctx));
    const vp_rs_state* st = reinterpret_cast<const vp_rs_state*>(hs);
    const uint8_t* mask = hs + off_mask;
    const float* pts = h_pts ? h_pts : reinterpret_cast<const float*>(hs + off_pts);
    const int taken = st->rounds * RS_ROUND < max_iters ? st->rounds * RS_ROUND : max_iters;
    int c = 0;
    for (int i = 0; i < n; i++) c += mask[i];
    const bool found = st->best_count >= P.m && vp_rs_refit(pts, pts + 2, 4, n, mask, model, model_out);
    if (!found) {
        c = 0;
        for (int k = 0; k < 9; k++) model_out[k] = 0.0;
    }
    if (inliers_host) {
        if (found) memcpy(inliers_host, mask, (size_t)n);
        else memset(inliers_host, 0, (size_t)n);
    }
    *n_inliers = c;
    *n_hypotheses = taken;
    return VP_OK;
}

extern "C" {

int vp_model_round_size(void) { return RS_ROUND; }
int vp_model_stage_points(void) { return RS_STAGE; }

int vp_estimate_model_f32(vp_ctx* ctx, const float* src_host, const float* dst_host, int n, int model, double threshold, int max_iters, double confidence,
                          uint32_t seed, double* model_out, uint8_t* inliers_host, int* n_inliers, int* n_hypotheses)
{
    if (const char* why = rs_check(src_host, dst_host, n, model, threshold, max_iters, confidence, model_out, n_inliers, n_hypotheses))
        return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    vp_rs_plan P;
    vp_rs_make_plan(n, model, max_iters, &P);
    vp_ws_frame W;
    uint8_t* d_ws; W.want(&d_ws, P.ws_bytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_estimate_model_f32"));
    // the packed form is made on the way into the pinned buffer the copy leaves from; the refit reads it there after the search
    const size_t pbytes = (size_t)n * 16;
    int slot = -1;
    float* hp = reinterpret_cast<float*>(vp_ring_take(ctx, pbytes, &slot));
    if (!hp) return vp_fail(ctx, VP_ERR_NOMEM, "pinned staging");
    for (int i = 0; i < n; i++) {
        hp[4 * (size_t)i] = src_host[2 * (size_t)i];
        hp[4 * (size_t)i + 1] = src_host[2 * (size_t)i + 1];
        hp[4 * (size_t)i + 2] = dst_host[2 * (size_t)i];
        hp[4 * (size_t)i + 3] = dst_host[2 * (size_t)i + 1];
    }
    int rc = h2d(ctx, d_ws, hp, pbytes);
    if (rc == VP_OK) rc = rs_run(ctx, P, d_ws, hp, n, model, threshold, max_iters, confidence, seed, model_out, inliers_host, n_inliers, n_hypotheses);
    vp_ring_done(ctx, slot);
    return rc;
}

int vp_estimate_model_dev(vp_ctx* ctx, const float* src_dev, const float* dst_dev, int n, int model, double threshold, int max_iters, double confidence,
                          uint32_t seed, double* model_out, uint8_t* inliers_host, int* n_inliers, int* n_hypotheses)
{
    if (const char* why = rs_check(src_dev, dst_dev, n, model, threshold, max_iters, confidence, model_out, n_inliers, n_hypotheses))
        return vp_fail(ctx, VP_ERR_INVALID, why);
    if ((uintptr_t)src_dev % 8 || (uintptr_t)dst_dev % 8) return vp_fail(ctx, VP_ERR_INVALID, "motion model: the device points are not 8-byte aligned");
    VP_TRY(check_ctx(ctx));
    vp_rs_plan P;
    vp_rs_make_plan(n, model, max_iters, &P);
    vp_ws_frame W;
    uint8_t* d_ws; W.want(&d_ws, P.ws_bytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_estimate_model_dev"));
    VP_TRY(vpk_rs_pack(ctx, src_dev, dst_dev, n, reinterpret_cast<float*>(d_ws)));
    return rs_run(ctx, P, d_ws, nullptr, n, model, threshold, max_iters, confidence, seed, model_out, inliers_host, n_inliers, n_hypotheses);
}

int vp_estimate_model_host(const float* src, const float* dst, int n, int model, double threshold, int max_iters, double confidence, uint32_t seed,
                           double* model_out, uint8_t* inliers /*nullable*/, int* n_inliers, int* n_hypotheses)
{
    if (const char* why = rs_check(src, dst, n, model, threshold, max_iters, confidence, model_out, n_inliers, n_hypotheses))
        return vp_fail(nullptr, VP_ERR_INVALID, why);
    std::vector<int32_t> need((size_t)vp_rs_round_count(max_iters));
    std::vector<uint8_t> mask((size_t)n);
    const int rounds = vp_rs_stop_table(n, model, confidence, max_iters, need.data());
    *n_inliers = vp_rs_search_host(src, dst, 2, n, model, threshold * threshold, max_iters, need.data(), rounds, seed, model_out, mask.data(), n_hypotheses);
    if (inliers) memcpy(inliers, mask.data(), (size_t)n);
    return VP_OK;
}

int vp_model_hypothesis(const float* src, const float* dst, int n, int model, uint32_t seed, int j, int32_t* sample, double* model_out)
{
    if (!src || !dst || !sample || !model_out) return vp_fail(nullptr, VP_ERR_INVALID, "motion model: a pointer is missing");
    if (const char* why = vp_rs_refusal(n, model, 1.0, 1, 0.5)) return vp_fail(nullptr, VP_ERR_INVALID, why);
    if (j < 0 || j >= RS_MAX_ITERS) return vp_fail(nullptr, VP_ERR_INVALID, "motion model: the hypothesis index must be 0 to 65535");
    return vp_rs_hypothesis(src, dst, 2, n, model, seed, (uint32_t)j, sample, model_out);
}

int vp_model_stop_table(int n, int model, double confidence, int max_iters, int32_t* need, int capacity, int* rounds)
{
    if (!need || !rounds) return vp_fail(nullptr, VP_ERR_INVALID, "motion model: a pointer is missing");
    if (const char* why = vp_rs_refusal(n, model, 1.0, max_iters, confidence)) return vp_fail(nullptr, VP_ERR_INVALID, why);
    if (capacity < vp_rs_round_count(max_iters)) return vp_fail(nullptr, VP_ERR_INVALID, "motion model: the table needs ceil(max_iters / round size) entries");
    *rounds = vp_rs_stop_table(n, model, confidence, max_iters, need);
    return VP_OK;
}

int vp_model_refit(const float* src, const float* dst, int n, const uint8_t* mask /*nullable*/, int model, double* model_out)
{
    if (!src || !dst || !model_out) return vp_fail(nullptr, VP_ERR_INVALID, "motion model: a pointer is missing");
    if (const char* why = vp_rs_refusal(n, model, 1.0, 1, 0.5)) return vp_fail(nullptr, VP_ERR_INVALID, why);
    return vp_rs_refit(src, dst, 2, n, mask, model, model_out);
}

}  // extern "C"
