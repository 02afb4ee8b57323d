// C ABI of libvp.so, robust plane fitting to the 3-D points of an image (kernels: vp_plane.hip; checks, point test, hypothesis,
// inlier test, stop rule, refit, host form and plan: vp_plane_plan.h), on host and device images, and the same statement as plain
// scalar C++.
#include "vp_api_util.h"
#include "vp_plane_plan.h"

int vpk_pl_run(vp_ctx* ctx, const vp_pl_plan& P, const vp_pl_buffers& B, const float* d_xyz, size_t xstride, int w, int h, const uint8_t* d_mask, size_t mstride,
               int metric, double t2, int max_iters, u32 seed, uint8_t* d_inl, size_t istride);

// everything the image entries refuse, from the arguments alone
static const char* plane_check(const float* xyz, size_t xstride, int w, int h, const int32_t* box, const uint8_t* mask, size_t mstride, int metric, double threshold,
                               int max_iters, double confidence, const uint8_t* inliers, size_t istride, const double* result, const int32_t* counts)
{
    if (!xyz || !result || !counts) return "fit plane: a pointer is missing";
    if (const char* why = vp_pl_size_refusal(w, h, box)) return why;
    if (xstride < (size_t)w * 12 || (mask && mstride < (size_t)w) || (inliers && istride < (size_t)w)) return "fit plane: a stride is below the row";
    if (xstride % 4) return "fit plane: the xyz stride is no multiple of 4";
    if ((uintptr_t)xyz % 4) return "fit plane: the xyz image is not aligned to its element size";
    if (const char* why = vp_pl_search_refusal(metric, threshold, max_iters, confidence)) return why;
    if (inliers) {
        const size_t ib = strided_bytes(istride, (size_t)w, h);
        if (dev_overlap(inliers, ib, xyz, strided_bytes(xstride, (size_t)w * 12, h))) return "fit plane: the inlier image overlaps xyz";
        if (mask && dev_overlap(inliers, ib, mask, strided_bytes(mstride, (size_t)w, h))) return "fit plane: the inlier image overlaps the mask";
    }
    return nullptr;
}

// the packed points (x, y, z, bits of the pixel index) of a host image, in raster order of the box
static void plane_points_host(const float* xyz, size_t xstride, int w, const vp_pl_box& b, const uint8_t* mask, size_t mstride, std::vector<float>* pts)
{
    for (int y = b.y0; y < b.y0 + b.rh; y++) {
        const float* row = reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(xyz) + (size_t)y * xstride);
        for (int x = b.x0; x < b.x0 + b.rw; x++) {
            if (mask && !mask[(size_t)y * mstride + x]) continue;
            const float* p = row + 3 * (size_t)x;
            if (!vp_pl_usable(p[0], p[1], p[2])) continue;
            const int32_t index = y * w + x;
            float bits;
            memcpy(&bits, &index, 4);
            pts->insert(pts->end(), {p[0], p[1], p[2], bits});
        }
    }
}

static void plane_answer(bool found, int k, const double* S, const double* M, int metric, int n_usable, int taken, int best_j, double* result, int32_t* counts)
{
    for (int i = 0; i < VP_PLANE_RESULT; i++) result[i] = 0.0;
    if (found) vp_pl_refit_close(k, S, M + 4, metric, M, result);
    counts[0] = n_usable;
    counts[1] = found ? k : 0;
    counts[2] = taken;
    counts[3] = found ? best_j : -1;
}

// device images in, the device inlier image (nullable) out, copied to h_inl (nullable, rows of w bytes) as well; enqueues every launch
// and synchronises once
static int plane_run(vp_ctx* ctx, const vp_pl_plan& P, const vp_pl_buffers& B, const float* d_xyz, size_t xstride, int w, int h, const uint8_t* d_mask, size_t mstride,
                     int metric, double threshold, int max_iters, double confidence, u32 seed, uint8_t* d_inl, size_t istride, uint8_t* h_inl, double* result, int32_t* counts)
{
    const size_t qbytes = (size_t)P.rounds * 8;
    int slot = -1;
    uint8_t* hq = vp_ring_take(ctx, qbytes, &slot);
    if (!hq) return vp_fail(ctx, VP_ERR_NOMEM, "pinned staging");
    vp_pl_stop_ratios(confidence, max_iters, reinterpret_cast<double*>(hq));
    int rc = h2d(ctx, B.qcrit, hq, qbytes);
    if (rc == VP_OK) rc = vpk_pl_run(ctx, P, B, d_xyz, xstride, w, h, d_mask, mstride, metric, threshold * threshold, max_iters, seed, d_inl, istride);
    vp_ring_done(ctx, slot);
    VP_TRY(rc);
    vp_pl_state* st = (vp_pl_state*)vp_hstage(ctx, sizeof(vp_pl_state));
    if (!st) return vp_fail(ctx, VP_ERR_NOMEM, "pinned staging");
    VP_TRY(d2h(ctx, st, B.state, sizeof(vp_pl_state)));
    if (h_inl) VP_TRY(d2h(ctx, h_inl, d_inl, (size_t)w * h));
    VP_TRY(vp_synchronize(ctx));
    const int taken = st->rounds * RS_ROUND < max_iters ? st->rounds * RS_ROUND : max_iters;
    plane_answer(st->best_count >= 3, st->best_count, st->sums, st->best, metric, st->n_usable, taken, st->best_j, result, counts);
    return VP_OK;
}

extern "C" {

int vp_fit_plane_plan(int w, int h, const int32_t* box, size_t* ws_bytes, int32_t* geometry)
{
    if (!ws_bytes || !geometry) return vp_fail(nullptr, VP_ERR_INVALID, "fit plane: a pointer is missing");
    if (const char* why = vp_pl_size_refusal(w, h, box)) return vp_fail(nullptr, VP_ERR_INVALID, why);
    vp_pl_plan P;
    vp_pl_make_plan(w, h, box, RS_MAX_ITERS, &P);
    vp_pl_buffers B;
    vp_ws_frame W;
    vp_pl_declare(W, P, &B);
    *ws_bytes = W.bytes();
    geometry[0] = PL_RUN;
    geometry[1] = PL_STAGE;
    geometry[2] = PL_HYP_PER_BLOCK;
    geometry[3] = PL_THREADS;
    geometry[4] = RS_ROUND;
    geometry[5] = P.ncand;
    geometry[6] = (int32_t)P.runs;
    geometry[7] = (int32_t)P.score_gy;
    return VP_OK;
}

int vp_fit_plane_dev(vp_ctx* ctx, const float* xyz_dev, size_t xyz_stride, int w, int h, const int32_t* box, const uint8_t* mask_dev, size_t mask_stride, int metric,
                     double threshold, int max_iters, double confidence, uint32_t seed, uint8_t* inliers_dev, size_t inliers_stride, double* result, int32_t* counts)
{
    if (const char* why = plane_check(xyz_dev, xyz_stride, w, h, box, mask_dev, mask_stride, metric, threshold, max_iters, confidence, inliers_dev, inliers_stride, result,
                                      counts))
        return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    vp_pl_plan P;
    vp_pl_make_plan(w, h, box, max_iters, &P);
    vp_pl_buffers B;
    vp_ws_frame W;
    vp_pl_declare(W, P, &B);
    VP_TRY(vp_ws_commit(ctx, W, "vp_fit_plane_dev"));
    return plane_run(ctx, P, B, xyz_dev, xyz_stride, w, h, mask_dev, mask_stride, metric, threshold, max_iters, confidence, seed, inliers_dev, inliers_stride, nullptr,
                     result, counts);
}

int vp_fit_plane_f32(vp_ctx* ctx, const float* xyz, int w, int h, const int32_t* box, const uint8_t* mask, int metric, double threshold, int max_iters, double confidence,
                     uint32_t seed, uint8_t* inliers, double* result, int32_t* counts)
{
    const size_t row = w > 0 ? (size_t)w : 0;
    if (const char* why = plane_check(xyz, row * 12, w, h, box, mask, row, metric, threshold, max_iters, confidence, inliers, row, result, counts))
        return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    vp_pl_plan P;
    vp_pl_make_plan(w, h, box, max_iters, &P);
    vp_pl_buffers B;
    vp_ws_frame W;
    vp_pl_declare(W, P, &B);
    float* d_xyz; W.want(&d_xyz, row * 12 * h);
    uint8_t* d_mask = nullptr; if (mask) W.want(&d_mask, row * h);
    uint8_t* d_inl = nullptr; if (inliers) W.want(&d_inl, row * h);
    VP_TRY(vp_ws_commit(ctx, W, "vp_fit_plane_f32"));
    VP_TRY(h2d(ctx, d_xyz, xyz, row * 12 * h));
    if (mask) VP_TRY(h2d(ctx, d_mask, mask, row * h));
    return plane_run(ctx, P, B, d_xyz, row * 12, w, h, d_mask, row, metric, threshold, max_iters, confidence, seed, d_inl, row, inliers, result, counts);
}

int vp_fit_plane_host(const float* xyz, size_t xyz_stride, int w, int h, const int32_t* box, const uint8_t* mask, size_t mask_stride, int metric, double threshold,
                      int max_iters, double confidence, uint32_t seed, uint8_t* inliers, size_t inliers_stride, double* result, int32_t* counts)
{
    if (const char* why = plane_check(xyz, xyz_stride, w, h, box, mask, mask_stride, metric, threshold, max_iters, confidence, inliers, inliers_stride, result, counts))
        return vp_fail(nullptr, VP_ERR_INVALID, why);
    vp_pl_plan P;
    vp_pl_make_plan(w, h, box, max_iters, &P);
    std::vector<float> pts;
    plane_points_host(xyz, xyz_stride, w, P.box, mask, mask_stride, &pts);
    const int n = (int)(pts.size() / 4);
    std::vector<uint8_t> keep((size_t)n + 1);
    double M[PL_MODEL], S[PL_SUMS];
    int taken = 0, best_j = -1;
    const int c = vp_pl_search_host(pts.data(), n, metric, threshold * threshold, max_iters, confidence, seed, M, keep.data(), &taken, &best_j);
    const int k = c >= 3 ? vp_pl_sums_host(pts.data(), n, keep.data(), M + 4, S) : 0;
    plane_answer(c >= 3, k, S, M, metric, n, taken, best_j, result, counts);
    if (inliers) {
        for (int y = 0; y < h; y++) memset(inliers + (size_t)y * inliers_stride, 0, (size_t)w);
        for (int i = 0; i < n; i++) {
            if (!keep[i]) continue;
            int32_t index;
            memcpy(&index, &pts[(size_t)i * 4 + 3], 4);
            inliers[(size_t)(index / w) * inliers_stride + (index % w)] = 255;
        }
    }
    return VP_OK;
}

int vp_plane_hypothesis(const float* pts4, int n, int metric, uint32_t seed, int j, int32_t* sample3, double* plane4)
{
    if (!pts4 || !sample3 || !plane4) return vp_fail(nullptr, VP_ERR_INVALID, "fit plane: a pointer is missing");
    if (n < 0 || n > PL_MAX_SIDE * PL_MAX_SIDE) return vp_fail(nullptr, VP_ERR_INVALID, "fit plane: at most 4096 x 4096 points");
    if (const char* why = vp_pl_search_refusal(metric, 1.0, 1, 0.5)) return vp_fail(nullptr, VP_ERR_INVALID, why);
    if (j < 0 || j >= RS_MAX_ITERS) return vp_fail(nullptr, VP_ERR_INVALID, "fit plane: the hypothesis index must be 0 to 65535");
    int32_t s[4];
    double M[PL_MODEL];
    const int ok = vp_pl_hypothesis(pts4, n, metric, seed, (uint32_t)j, s, M);
    for (int k = 0; k < 3; k++) sample3[k] = s[k];
    for (int k = 0; k < 4; k++) plane4[k] = M[k];
    return ok;
}

int vp_plane_refit(const float* pts4, int n, const uint8_t* keep /*nullable*/, int metric, double* result)
{
    if (!pts4 || !result) return vp_fail(nullptr, VP_ERR_INVALID, "fit plane: a pointer is missing");
    if (n < 0 || n > PL_MAX_SIDE * PL_MAX_SIDE) return vp_fail(nullptr, VP_ERR_INVALID, "fit plane: at most 4096 x 4096 points");
    if (const char* why = vp_pl_search_refusal(metric, 1.0, 1, 0.5)) return vp_fail(nullptr, VP_ERR_INVALID, why);
    for (int i = 0; i < VP_PLANE_RESULT; i++) result[i] = 0.0;
    int first = 0;
    while (first < n && keep && !keep[first]) first++;
    if (first >= n) return 0;
    const double p0[3] = {(double)pts4[(size_t)first * 4], (double)pts4[(size_t)first * 4 + 1], (double)pts4[(size_t)first * 4 + 2]};
    double S[PL_SUMS];
    const int k = vp_pl_sums_host(pts4, n, keep, p0, S);
    return vp_pl_refit_close(k, S, p0, metric, nullptr, result);
}

}  // extern "C"
