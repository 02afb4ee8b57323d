// C ABI of libvp.so, features: FAST-9 corners (cv2.FastFeatureDetector, TYPE_9_16), the library's steered 256-bit binary descriptor and
// the brute-force Hamming matcher (cv2.BFMatcher(NORM_HAMMING)) on host and device arrays (kernels: vp_features.hip; checks, plans,
// tables and the pattern rule: vp_features_plan.h).
#include "vp_api_util.h"
#include "vp_features_plan.h"

namespace {

// the 32 steered patterns and the taps of B's blur (x taps, then y taps), made once per process; every context uploads its own copy
struct ft_host_table {
    int8_t pattern[FT_PATTERN_BYTES];
    uint16_t taps[16];
    int ok;
};

const ft_host_table& ft_table()
{
    static const ft_host_table T = [] {
        ft_host_table t;
        memset(&t, 0, sizeof t);
        t.ok = vp_ft_build_pattern(t.pattern) == 0;
        vp_gaussian_taps(FT_BLUR_K, FT_BLUR_SIGMA, t.taps);
        vp_gaussian_taps(FT_BLUR_K, FT_BLUR_SIGMA, t.taps + FT_BLUR_K);
        return t;
    }();
    return T;
}

int ft_pattern_ready(vp_ctx* ctx)
{
    if (ctx->ft.pattern) return VP_OK;
    const ft_host_table& T = ft_table();
    if (!T.ok) return vp_fail(ctx, VP_ERR_INVALID, "describe: a steered pattern coordinate leaves -15 .. 15");
    int8_t* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, FT_PATTERN_BYTES + sizeof T.taps);
    if (e != hipSuccess) return vp_fail(ctx, VP_ERR_NOMEM, "describe: the pattern table", e);
    e = hipMemcpyAsync(d, T.pattern, FT_PATTERN_BYTES + sizeof T.taps, hipMemcpyHostToDevice, ctx->stream);   // pattern and taps are adjacent members
    if (e != hipSuccess) { (void)hipFree(d); return vp_fail(ctx, VP_ERR_HIP, "describe: the pattern upload", e); }
    ctx->ft.pattern = d;
    return VP_OK;
}
static_assert(offsetof(ft_host_table, taps) == FT_PATTERN_BYTES, "the taps follow the pattern");

// the launches, then the count, then as many corners as the caller has room for; d_ws: P.ws_bytes, reserved by the caller
int fast_run(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int threshold, int nonmax, const vp_fast_plan& P, uint8_t* d_ws, int32_t* xy_host,
             int32_t* score_host, int* n_found)
{
    VP_TRY(vpk_fast(ctx, d_src, stride, w, h, threshold, nonmax != 0, P, d_ws));
    u32* hs = (u32*)vp_hstage(ctx, 16);
    if (!hs) return vp_fail(ctx, VP_ERR_NOMEM, "pinned staging");
    VP_TRY(d2h(ctx, hs, d_ws + P.off_cnt + P.chunks * 4, 4));
    VP_TRY(vp_synchronize(ctx));
    const size_t total = hs[0];
    if (total > P.max_found) return vp_fail(ctx, VP_ERR_HIP, "FAST: corner count above its bound");
    const size_t m = total < P.out_cap ? total : P.out_cap;
    if (m) {
        VP_TRY(d2h(ctx, xy_host, d_ws + P.off_xy, m * 8));
        VP_TRY(d2h(ctx, score_host, d_ws + P.off_val, m * 4));
        VP_TRY(vp_synchronize(ctx));
    }
    *n_found = (int)total;
    return VP_OK;
}

// B into the workspace with the existing two-pass blur, the points over in a pinned chunk of the context's ring, one launch, results back
int describe_run(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, const float* pts, int n, const vp_describe_plan& P, uint8_t* d_ws, uint8_t* desc,
                 uint8_t* bin, uint8_t* status)
{
    VP_TRY(ft_pattern_ready(ctx));
    const uint16_t* d_taps = reinterpret_cast<const uint16_t*>(ctx->ft.pattern + FT_PATTERN_BYTES);
    uint8_t* d_blur = d_ws + P.off_blur;
    float* d_pts = reinterpret_cast<float*>(d_ws + P.off_pts);
    VP_TRY(vpk_gaussian_blur(ctx, d_src, w, h, 1, d_taps, FT_BLUR_K, FT_BLUR_K, reinterpret_cast<uint16_t*>(d_ws + P.off_tmp), d_blur, stride));
    const size_t pbytes = (size_t)n * 8;
    int slot = -1;
    uint8_t* hp = vp_ring_take(ctx, pbytes, &slot);
    if (!hp) return vp_fail(ctx, VP_ERR_NOMEM, "pinned staging");
    memcpy(hp, pts, pbytes);
    int rc = h2d(ctx, d_pts, hp, pbytes);
    if (rc == VP_OK)
        rc = vpk_describe(ctx, d_src, stride, d_blur, w, h, d_pts, n, ctx->ft.pattern, P.grid, d_ws + P.off_desc, d_ws + P.off_bin, d_ws + P.off_status);
    vp_ring_done(ctx, slot);
    VP_TRY(rc);
    VP_TRY(d2h(ctx, desc, d_ws + P.off_desc, (size_t)n * FT_DESC_BYTES));
    VP_TRY(d2h(ctx, bin, d_ws + P.off_bin, (size_t)n));
    VP_TRY(d2h(ctx, status, d_ws + P.off_status, (size_t)n));
    return vp_synchronize(ctx);
}

// Level 0 from d_src (device rows of stride bytes) or h_src (host rows), the other levels by the resize kernel, each from the one
// before, every level's B by the two-pass blur; then vpk_pyr_features, whose launches do not depend on the number of levels; the whole
// capacity of every list comes back, so the one synchronisation is the last thing queued.  P: at least one level, capacity >= 1.
int pyr_run(vp_ctx* ctx, const uint8_t* d_src, const uint8_t* h_src, size_t stride, int w, int h, int threshold, const vp_pyr_plan& P, float* xy0_host, int32_t* lxy_host,
            int32_t* score_host, uint8_t* bin_host, uint8_t* desc_host, uint8_t* desc_dev, int* n_found)
{
    VP_TRY(ft_pattern_ready(ctx));
    const uint16_t* d_taps = reinterpret_cast<const uint16_t*>(ctx->ft.pattern + FT_PATTERN_BYTES);
    vp_ws_frame W;
    uint8_t* d_ws; W.want(&d_ws, P.ws_bytes);
    VP_TRY(vp_ws_commit(ctx, W, "pyr_run"));
    const vp_pyr_table& T = P.T;
    uint8_t* d_img = d_ws + P.off_img;
    if (h_src) {
        VP_TRY(h2d_rows(ctx, d_img, (size_t)w, h_src, stride, (size_t)w, h));
    } else {
        VP_HIP(ctx, hipMemcpy2DAsync(d_img, (size_t)w, d_src, stride, (size_t)w, h, hipMemcpyDeviceToDevice, ctx->stream));
    }
    for (int l = 1; l < T.n_levels; l++) {
        const vp_pyr_level &A = T.L[l - 1], &B = T.L[l];
        VP_TRY(vpk_resize_u8(ctx, d_img + A.off, A.w, A.h, 1, B.w, B.h, (double)B.w / A.w, (double)B.h / A.h, d_img + B.off));
    }
    for (int l = 0; l < T.n_levels; l++)
        VP_TRY(vpk_gaussian_blur(ctx, d_img + T.L[l].off, T.L[l].w, T.L[l].h, 1, d_taps, FT_BLUR_K, FT_BLUR_K, reinterpret_cast<uint16_t*>(d_ws + P.off_tmp),
                                 d_ws + P.off_blur + T.L[l].off));
    uint8_t* d_desc = desc_dev ? desc_dev : d_ws + P.off_desc;
    VP_TRY(vpk_pyr_features(ctx, P, threshold, ctx->ft.pattern, d_ws, d_desc));
    u32* hs = (u32*)vp_hstage(ctx, 16);
    if (!hs) return vp_fail(ctx, VP_ERR_NOMEM, "pinned staging");
    VP_TRY(d2h(ctx, hs, d_ws + P.off_gt + P.chunks * 4, 4));
    VP_TRY(d2h(ctx, lxy_host, d_ws + P.off_lxy, P.cap * 12));
    VP_TRY(d2h(ctx, score_host, d_ws + P.off_val, P.cap * 4));
    VP_TRY(d2h(ctx, bin_host, d_ws + P.off_bin, P.cap));
    VP_TRY(d2h(ctx, desc_host, d_desc, P.cap * FT_DESC_BYTES));
    VP_TRY(vp_synchronize(ctx));
    const size_t n = hs[0];
    if (n > P.cap) return vp_fail(ctx, VP_ERR_HIP, "pyramid features: point count above the capacity");
    for (size_t i = 0; i < n; i++) {
        const int32_t l = lxy_host[3 * i];
        if (l < 0 || l >= T.n_levels) return vp_fail(ctx, VP_ERR_HIP, "pyramid features: a point's level is outside the pyramid");
        // level 0 coordinates in double, in this order, rounded to float32 once (the compile has no contraction)
        xy0_host[2 * i] = (float)(((double)lxy_host[3 * i + 1] + 0.5) * ((double)w / T.L[l].w) - 0.5);
        xy0_host[2 * i + 1] = (float)(((double)lxy_host[3 * i + 2] + 0.5) * ((double)h / T.L[l].h) - 0.5);
    }
    *n_found = (int)n;
    return VP_OK;
}

// what both forms of vp_pyr_features_* check before they need a device; *P is made when NULL comes back
const char* pyr_checks(const void* src, size_t stride, int w, int h, int levels, int threshold, int max_points, const float* xy0, const int32_t* lxy, const int32_t* score,
                       const uint8_t* bin, const uint8_t* desc, const uint8_t* desc_dev, const int* n_found, vp_pyr_plan* P)
{
    if (!src || !n_found || (max_points > 0 && (!xy0 || !lxy || !score || !bin || !desc))) return "pyramid features: a pointer is missing";
    if (const char* why = vp_pyr_refusal(w, h, stride, levels, threshold, max_points)) return why;
    if ((uintptr_t)desc_dev % 8) return "pyramid features: the device descriptors must be 8-byte aligned";
    vp_pyr_make_plan(w, h, levels, max_points, P);
    return nullptr;
}

// workspace of a matcher call beyond what the caller stages: the partial results of both directions and the reverse matches
struct hamming_bufs { void *part, *rpart; int32_t *rev, *rdist; };
void hamming_want(vp_ws_frame& W, const vp_hamming_plan_t& P, const vp_hamming_plan_t& R, int nt, int cross_check, hamming_bufs* b)
{
    b->part = b->rpart = nullptr;
    if (P.partial_bytes) W.want(&b->part, P.partial_bytes);
    if (!cross_check) return;
    if (R.partial_bytes) W.want(&b->rpart, R.partial_bytes);
    W.want(&b->rev, (size_t)nt * 4);
    W.want(&b->rdist, (size_t)nt * 4);
}

// nq, nt >= 1
int hamming_run(vp_ctx* ctx, const uint8_t* d_q, size_t qstride, int nq, const uint8_t* d_t, size_t tstride, int nt, const vp_hamming_plan_t& P,
                const vp_hamming_plan_t& R, int k, int cross_check, int32_t* d_idx, int32_t* d_dist, const hamming_bufs& b)
{
    VP_TRY(vpk_hamming_knn(ctx, d_q, qstride, nq, d_t, tstride, nt, P, k, d_idx, d_dist, b.part));
    if (!cross_check) return VP_OK;
    VP_TRY(vpk_hamming_knn(ctx, d_t, tstride, nt, d_q, qstride, nq, R, 1, b.rev, b.rdist, b.rpart));
    return vpk_hamming_cross(ctx, d_idx, b.rev, nq);
}

}  // namespace

void vp_features_teardown(vp_ctx* ctx)
{
    if (ctx->ft.pattern) (void)hipFree(ctx->ft.pattern);
    ctx->ft.pattern = nullptr;
}

extern "C" {

int vp_fast_u8(vp_ctx* ctx, const uint8_t* src, size_t stride, int w, int h, int threshold, int nonmax, int32_t* xy_host, int32_t* score_host, int capacity,
               int* n_found)
{
    if (!src || !n_found || (capacity > 0 && (!xy_host || !score_host))) return vp_fail(ctx, VP_ERR_INVALID, "vp_fast_u8: a pointer is missing");
    if (const char* why = vp_fast_refusal(w, h, stride, threshold, capacity)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    vp_fast_plan P;
    vp_fast_make_plan(w, h, capacity, &P);
    const size_t npx = (size_t)w * h;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, npx);
    uint8_t* d_ws; W.want(&d_ws, P.ws_bytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_fast_u8"));
    VP_TRY(h2d_rows(ctx, d_src, (size_t)w, src, stride, (size_t)w, h));
    return fast_run(ctx, d_src, (size_t)w, w, h, threshold, nonmax, P, d_ws, xy_host, score_host, n_found);
}

int vp_fast_dev(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int threshold, int nonmax, int32_t* xy_host, int32_t* score_host, int capacity,
                int* n_found)
{
    if (!d_src || !n_found || (capacity > 0 && (!xy_host || !score_host))) return vp_fail(ctx, VP_ERR_INVALID, "vp_fast_dev: a pointer is missing");
    if (const char* why = vp_fast_refusal(w, h, stride, threshold, capacity)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    vp_fast_plan P;
    vp_fast_make_plan(w, h, capacity, &P);
    vp_ws_frame W;
    uint8_t* d_ws; W.want(&d_ws, P.ws_bytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_fast_dev"));
    return fast_run(ctx, d_src, stride, w, h, threshold, nonmax, P, d_ws, xy_host, score_host, n_found);
}

int vp_describe_pattern(int8_t* out)
{
    if (!out) return vp_fail(nullptr, VP_ERR_INVALID, "vp_describe_pattern: a pointer is missing");
    const ft_host_table& T = ft_table();
    if (!T.ok) return vp_fail(nullptr, VP_ERR_INVALID, "describe: a steered pattern coordinate leaves -15 .. 15");
    memcpy(out, T.pattern, FT_PATTERN_BYTES);
    return VP_OK;
}

int vp_describe_u8(vp_ctx* ctx, const uint8_t* src, size_t stride, int w, int h, const float* pts, int n, uint8_t* desc, uint8_t* bin, uint8_t* status)
{
    if (!src || (n > 0 && (!pts || !desc || !bin || !status))) return vp_fail(ctx, VP_ERR_INVALID, "vp_describe_u8: a pointer is missing");
    if (const char* why = vp_describe_refusal(w, h, stride, n)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    if (n == 0) return VP_OK;
    vp_describe_plan P;
    vp_describe_make_plan(w, h, n, &P);
    const size_t npx = (size_t)w * h;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, npx);
    uint8_t* d_ws; W.want(&d_ws, P.ws_bytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_describe_u8"));
    VP_TRY(h2d_rows(ctx, d_src, (size_t)w, src, stride, (size_t)w, h));
    return describe_run(ctx, d_src, (size_t)w, w, h, pts, n, P, d_ws, desc, bin, status);
}

int vp_describe_dev(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, const float* pts, int n, uint8_t* desc, uint8_t* bin, uint8_t* status)
{
    if (!d_src || (n > 0 && (!pts || !desc || !bin || !status))) return vp_fail(ctx, VP_ERR_INVALID, "vp_describe_dev: a pointer is missing");
    if (const char* why = vp_describe_refusal(w, h, stride, n)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    if (n == 0) return VP_OK;
    vp_describe_plan P;
    vp_describe_make_plan(w, h, n, &P);
    vp_ws_frame W;
    uint8_t* d_ws; W.want(&d_ws, P.ws_bytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_describe_dev"));
    return describe_run(ctx, d_src, stride, w, h, pts, n, P, d_ws, desc, bin, status);
}

int vp_pyr_features_plan(int w, int h, int levels, int max_points, int* n_levels, int32_t* level_wh, int32_t* quota)
{
    if (!n_levels || !level_wh || !quota) return vp_fail(nullptr, VP_ERR_INVALID, "vp_pyr_features_plan: a pointer is missing");
    if (const char* why = vp_pyr_refusal(w, h, (size_t)(w > 0 ? w : 0), levels, 0, max_points)) return vp_fail(nullptr, VP_ERR_INVALID, why);
    vp_pyr_plan P;
    vp_pyr_make_plan(w, h, levels, max_points, &P);
    *n_levels = P.T.n_levels;
    for (int l = 0; l < P.T.n_levels; l++) {
        level_wh[2 * l] = P.T.L[l].w;
        level_wh[2 * l + 1] = P.T.L[l].h;
        quota[l] = (int32_t)P.T.L[l].quota;
    }
    return VP_OK;
}

int vp_pyr_features_u8(vp_ctx* ctx, const uint8_t* src, size_t stride, int w, int h, int levels, int threshold, int max_points, float* xy0_host, int32_t* lxy_host,
                       int32_t* score_host, uint8_t* bin_host, uint8_t* desc_host, uint8_t* desc_dev, int* n_found)
{
    vp_pyr_plan P;
    if (const char* why = pyr_checks(src, stride, w, h, levels, threshold, max_points, xy0_host, lxy_host, score_host, bin_host, desc_host, desc_dev, n_found, &P))
        return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    *n_found = 0;
    if (max_points == 0 || P.T.n_levels == 0) return VP_OK;
    return pyr_run(ctx, nullptr, src, stride, w, h, threshold, P, xy0_host, lxy_host, score_host, bin_host, desc_host, desc_dev, n_found);
}

int vp_pyr_features_dev(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int levels, int threshold, int max_points, float* xy0_host, int32_t* lxy_host,
                        int32_t* score_host, uint8_t* bin_host, uint8_t* desc_host, uint8_t* desc_dev, int* n_found)
{
    vp_pyr_plan P;
    if (const char* why = pyr_checks(d_src, stride, w, h, levels, threshold, max_points, xy0_host, lxy_host, score_host, bin_host, desc_host, desc_dev, n_found, &P))
        return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    *n_found = 0;
    if (max_points == 0 || P.T.n_levels == 0) return VP_OK;
    return pyr_run(ctx, d_src, nullptr, stride, w, h, threshold, P, xy0_host, lxy_host, score_host, bin_host, desc_host, desc_dev, n_found);
}

int vp_hamming_plan(int nq, int nt, int D, int* query_tiles, int* train_splits)
{
    if (!query_tiles || !train_splits) return vp_fail(nullptr, VP_ERR_INVALID, "vp_hamming_plan: a pointer is missing");
    if (const char* why = vp_hamming_refusal(nq, nt, D, (size_t)HM_MAX_D, (size_t)HM_MAX_D, 1, 0)) return vp_fail(nullptr, VP_ERR_INVALID, why);
    vp_hamming_plan_t P;
    vp_hamming_make_plan(nq, nt, D, &P);
    *query_tiles = P.query_tiles;
    *train_splits = P.train_splits;
    return VP_OK;
}

int vp_hamming_knn_u8(vp_ctx* ctx, const uint8_t* query, size_t qstride, int nq, const uint8_t* train, size_t tstride, int nt, int D, int k, int cross_check,
                      int32_t* idx, int32_t* dist)
{
    if ((nq > 0 && (!query || !idx || !dist)) || (nt > 0 && !train)) return vp_fail(ctx, VP_ERR_INVALID, "vp_hamming_knn_u8: a pointer is missing");
    if (const char* why = vp_hamming_refusal(nq, nt, D, qstride, tstride, k, cross_check)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    if (nq == 0) return VP_OK;
    const size_t obytes = (size_t)nq * k * 4;
    if (nt == 0) {                                                       // no neighbour at all: every entry is -1
        memset(idx, 0xff, obytes);
        memset(dist, 0xff, obytes);
        return VP_OK;
    }
    vp_hamming_plan_t P, R;
    vp_hamming_make_plan(nq, nt, D, &P);
    vp_hamming_make_plan(nt, nq, D, &R);
    const size_t qbytes = (size_t)nq * D, tbytes = (size_t)nt * D;
    vp_ws_frame W;
    uint8_t* d_q; W.want(&d_q, qbytes);
    uint8_t* d_t; W.want(&d_t, tbytes);
    int32_t* d_idx; W.want(&d_idx, obytes);
    int32_t* d_dist; W.want(&d_dist, obytes);
    hamming_bufs b;
    hamming_want(W, P, R, nt, cross_check, &b);
    VP_TRY(vp_ws_commit(ctx, W, "vp_hamming_knn_u8"));
    VP_TRY(h2d_rows(ctx, d_q, (size_t)D, query, qstride, (size_t)D, nq));
    VP_TRY(h2d_rows(ctx, d_t, (size_t)D, train, tstride, (size_t)D, nt));
    VP_TRY(hamming_run(ctx, d_q, (size_t)D, nq, d_t, (size_t)D, nt, P, R, k, cross_check, d_idx, d_dist, b));
    VP_TRY(d2h(ctx, idx, d_idx, obytes));
    VP_TRY(d2h(ctx, dist, d_dist, obytes));
    return vp_synchronize(ctx);
}

int vp_hamming_knn_dev(vp_ctx* ctx, const uint8_t* d_query, size_t qstride, int nq, const uint8_t* d_train, size_t tstride, int nt, int D, int k, int cross_check,
                       int32_t* d_idx, int32_t* d_dist)
{
    if ((nq > 0 && (!d_query || !d_idx || !d_dist)) || (nt > 0 && !d_train)) return vp_fail(ctx, VP_ERR_INVALID, "vp_hamming_knn_dev: a pointer is missing");
    if (const char* why = vp_hamming_refusal(nq, nt, D, qstride, tstride, k, cross_check)) return vp_fail(ctx, VP_ERR_INVALID, why);
    if ((uintptr_t)d_query % 8 || (uintptr_t)d_train % 8 || (uintptr_t)d_idx % 4 || (uintptr_t)d_dist % 4)
        return vp_fail(ctx, VP_ERR_INVALID, "vp_hamming_knn_dev: the descriptors must be 8-byte aligned, the results 4-byte aligned");
    VP_TRY(check_ctx(ctx));
    if (nq == 0) return VP_OK;
    const size_t obytes = (size_t)nq * k * 4;
    if (nt == 0) {
        VP_HIP(ctx, hipMemsetAsync(d_idx, 0xff, obytes, ctx->stream));
        VP_HIP(ctx, hipMemsetAsync(d_dist, 0xff, obytes, ctx->stream));
        return VP_OK;
    }
    vp_hamming_plan_t P, R;
    vp_hamming_make_plan(nq, nt, D, &P);
    vp_hamming_make_plan(nt, nq, D, &R);
    vp_ws_frame W;
    hamming_bufs b;
    hamming_want(W, P, R, nt, cross_check, &b);
    VP_TRY(vp_ws_commit(ctx, W, "vp_hamming_knn_dev"));
    return hamming_run(ctx, d_query, qstride, nq, d_train, tstride, nt, P, R, k, cross_check, d_idx, d_dist, b);
}

}  // extern "C"
