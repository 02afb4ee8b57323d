// C ABI of libvp.so, sparse optical flow: cv2.calcOpticalFlowPyrLK on device pyramids and on host images (kernel: vp_flow.hip; checks,
// level rule and LDS layout: vp_flow_plan.h).
#include "vp_api_util.h"
#include "vp_flow_plan.h"

#define LK_OUT_BYTES 16      // per point: x, y, err (float32), status (uint32)

// the points (and the guesses) go over in a pinned chunk of the context's ring, the launch follows; synchronises only for out_host
static int lk_run(vp_ctx* ctx, const vp_lk_levels& L, const vp_lk_plan& P, const float* prev_pts, const float* init_pts, int n, int win_w, int win_h, int max_count,
                  double eps, int flags, double min_eig, float* d_pts, u32* d_res, void* out_host)
{
    const size_t pbytes = (size_t)n * 8, both = init_pts ? 2 * pbytes : pbytes;
    int slot = -1;
    uint8_t* hp = vp_ring_take(ctx, both, &slot);
    if (!hp) return vp_fail(ctx, VP_ERR_NOMEM, "pinned staging");
    memcpy(hp, prev_pts, pbytes);
    if (init_pts) memcpy(hp + pbytes, init_pts, pbytes);
    int rc = h2d(ctx, d_pts, hp, both);
    if (rc == VP_OK)
        rc = vpk_lk_flow(ctx, L, P, win_w, win_h, vp_lk_max_count(max_count), vp_lk_eps2(eps), flags, min_eig, d_pts, init_pts ? d_pts + 2 * (size_t)n : nullptr, d_res);
    vp_ring_done(ctx, slot);
    if (rc != VP_OK || !out_host) return rc;
    VP_TRY(d2h(ctx, out_host, d_res, (size_t)n * LK_OUT_BYTES));
    return vp_synchronize(ctx);
}

extern "C" {

int vp_lk_flow_levels(int w, int h, int win_w, int win_h, int max_level)
{
    if (w < 1 || h < 1 || win_w < 1 || win_h < 1 || max_level < 0) return 0;
    return vp_lk_level_count(w, h, win_w, win_h, max_level);
}

int vp_lk_flow_dev(vp_ctx* ctx, const uint8_t* const* prev_levels, const size_t* prev_strides, const uint8_t* const* next_levels, const size_t* next_strides,
                   int n_levels, int w, int h, const float* prev_pts, const float* init_pts, int n, int win_w, int win_h, int max_level, int max_count, double eps,
                   int flags, double min_eig_threshold, void* d_out, void* out_host)
{
    if (!prev_levels || !prev_strides || !next_levels || !next_strides || !prev_pts || (!d_out && !out_host))
        return vp_fail(ctx, VP_ERR_INVALID, "vp_lk_flow_dev: a pointer is missing");
    if (const char* why = vp_lk_refusal(w, h, win_w, win_h, n, max_level, max_count, eps, flags, min_eig_threshold)) return vp_fail(ctx, VP_ERR_INVALID, why);
    if ((flags & LK_USE_INITIAL_FLOW) && !init_pts) return vp_fail(ctx, VP_ERR_INVALID, "vp_lk_flow_dev: a pointer is missing (the initial flow)");
    if (n_levels < 1 || n_levels > LK_MAX_LEVELS) return vp_fail(ctx, VP_ERR_INVALID, "optical flow: 1 to 16 pyramid levels");
    vp_lk_plan P;
    vp_lk_make_plan(w, h, win_w, win_h, n, max_level < n_levels - 1 ? max_level : n_levels - 1, &P);
    if (d_out && (uintptr_t)d_out % 4) return vp_fail(ctx, VP_ERR_INVALID, "vp_lk_flow_dev: the result is not 4-byte aligned");
    vp_lk_levels L;
    memset(&L, 0, sizeof L);
    for (int l = 0; l < P.levels; l++) {
        if (!prev_levels[l] || !next_levels[l]) return vp_fail(ctx, VP_ERR_INVALID, "vp_lk_flow_dev: a pointer is missing (a pyramid level)");
        if (prev_strides[l] < (size_t)P.cols[l] || next_strides[l] < (size_t)P.cols[l]) return vp_fail(ctx, VP_ERR_INVALID, "optical flow: a stride is below the row");
        if (d_out && (dev_overlap(prev_levels[l], strided_bytes(prev_strides[l], (size_t)P.cols[l], P.rows[l]), d_out, (size_t)n * LK_OUT_BYTES) ||
                      dev_overlap(next_levels[l], strided_bytes(next_strides[l], (size_t)P.cols[l], P.rows[l]), d_out, (size_t)n * LK_OUT_BYTES)))
            return vp_fail(ctx, VP_ERR_INVALID, "vp_lk_flow_dev: the result overlaps a pyramid level");
        L.prev[l] = prev_levels[l];
        L.next[l] = next_levels[l];
        L.prev_stride[l] = prev_strides[l];
        L.next_stride[l] = next_strides[l];
        L.cols[l] = P.cols[l];
        L.rows[l] = P.rows[l];
    }
    VP_TRY(check_ctx(ctx));
    const size_t pbytes = (size_t)n * 8, obytes = (size_t)n * LK_OUT_BYTES;
    vp_ws_frame W;
    float* d_pts; W.want(&d_pts, 2 * pbytes);
    u32* d_res = (u32*)d_out;
    if (!d_res) W.want(&d_res, obytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_lk_flow_dev"));
    return lk_run(ctx, L, P, prev_pts, (flags & LK_USE_INITIAL_FLOW) ? init_pts : nullptr, n, win_w, win_h, max_count, eps, flags, min_eig_threshold, d_pts, d_res,
                  out_host);
}

int vp_lk_flow_u8(vp_ctx* ctx, const uint8_t* prev, const uint8_t* next, int w, int h, const float* prev_pts, const float* init_pts, int n, int win_w, int win_h,
                  int max_level, int max_count, double eps, int flags, double min_eig_threshold, void* out_host)
{
    if (!prev || !next || !prev_pts || !out_host) return vp_fail(ctx, VP_ERR_INVALID, "vp_lk_flow_u8: a pointer is missing");
    if (const char* why = vp_lk_refusal(w, h, win_w, win_h, n, max_level, max_count, eps, flags, min_eig_threshold)) return vp_fail(ctx, VP_ERR_INVALID, why);
    if ((flags & LK_USE_INITIAL_FLOW) && !init_pts) return vp_fail(ctx, VP_ERR_INVALID, "vp_lk_flow_u8: a pointer is missing (the initial flow)");
    VP_TRY(check_ctx(ctx));
    vp_lk_plan P;
    vp_lk_make_plan(w, h, win_w, win_h, n, max_level, &P);
    const size_t pbytes = (size_t)n * 8, obytes = (size_t)n * LK_OUT_BYTES;
    vp_ws_frame W;
    float* d_pts; W.want(&d_pts, 2 * pbytes);
    u32* d_res; W.want(&d_res, obytes);
    vp_lk_levels L;
    memset(&L, 0, sizeof L);
    for (int l = 0; l < P.levels; l++) {
        W.want(&L.prev[l], (size_t)P.cols[l] * P.rows[l]);
        W.want(&L.next[l], (size_t)P.cols[l] * P.rows[l]);
    }
    VP_TRY(vp_ws_commit(ctx, W, "vp_lk_flow_u8"));
    for (int l = 0; l < P.levels; l++) {
        const size_t bytes = (size_t)P.cols[l] * P.rows[l];
        uint8_t *d_p = const_cast<uint8_t*>(L.prev[l]), *d_n = const_cast<uint8_t*>(L.next[l]);
        if (l == 0) {
            VP_TRY(h2d(ctx, d_p, prev, bytes));
            VP_TRY(h2d(ctx, d_n, next, bytes));
        } else {
            VP_TRY(vp_pyr_down_dev(ctx, L.prev[l - 1], (size_t)P.cols[l - 1], P.cols[l - 1], P.rows[l - 1], 1, VP_BORDER_REFLECT_101, d_p));
            VP_TRY(vp_pyr_down_dev(ctx, L.next[l - 1], (size_t)P.cols[l - 1], P.cols[l - 1], P.rows[l - 1], 1, VP_BORDER_REFLECT_101, d_n));
        }
        L.prev_stride[l] = L.next_stride[l] = (size_t)P.cols[l];
        L.cols[l] = P.cols[l];
        L.rows[l] = P.rows[l];
    }
    return lk_run(ctx, L, P, prev_pts, (flags & LK_USE_INITIAL_FLOW) ? init_pts : nullptr, n, win_w, win_h, max_count, eps, flags, min_eig_threshold, d_pts, d_res,
                  out_host);
}

}  // extern "C"
