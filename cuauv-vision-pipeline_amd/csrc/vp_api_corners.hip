// C ABI of libvp.so, corners: the response maps of cv2.cornerMinEigenVal / cornerHarris and the selection of cv2.goodFeaturesToTrack
// on host and device images (kernels: vp_corners.hip; checks, tile and the greedy pass: vp_corners_plan.h).
#include "vp_api_util.h"
#include "vp_corners_plan.h"

// Response, maximum, candidates and their order on the device; the count comes back, then the ordered words, and the greedy pass runs
// here.  d_mask (rows of mstride bytes) and d_bits (the mask's bit plane) are nullable device pointers; the caller's frame holds b
// beside what it staged.
struct gf_bufs { float* resp; u64 *k0, *k1; u32* cnt; };
static void gf_want(vp_ws_frame& W, int w, int h, gf_bufs* b)
{
    if (w < 3 || h < 3) return;                                  // good_features_run launches nothing
    const size_t npx = (size_t)w * h, kcap = (size_t)(w - 2) * (h - 2);
    W.want(&b->resp, npx * 4);
    W.want(&b->k0, kcap * 8);
    W.want(&b->k1, kcap * 8);
    W.want(&b->cnt, 8);
}
static int good_features_run(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int max_corners, double quality, double min_distance,
                             const uint8_t* d_mask, size_t mstride, const u64* d_bits, int block_size, int harris, double k, float* corners,
                             int capacity, int* n_corners, const gf_bufs& b)
{
    *n_corners = 0;
    if (w < 3 || h < 3) return VP_OK;                            // no interior pixel: cv2 returns nothing
    const size_t kcap = (size_t)(w - 2) * (h - 2);
    float* d_resp = b.resp;
    u64 *d_k0 = b.k0, *d_k1 = b.k1;
    u32* d_cnt = b.cnt;
    VP_TRY(vpk_corner_response(ctx, d_src, stride, w, h, block_size, harris, k, VP_BORDER_REFLECT_101, d_resp));
    VP_TRY(vpk_corner_candidates(ctx, d_resp, w, h, d_mask, mstride, d_bits, quality, d_cnt, d_k0, kcap));
    u32* hs = (u32*)vp_hstage(ctx, 16);
    if (!hs) return vp_fail(ctx, VP_ERR_NOMEM, "pinned staging");
    VP_TRY(d2h(ctx, hs, d_cnt, 8));
    VP_TRY(vp_synchronize(ctx));
    const u32 ncand = hs[1];
    if (ncand == 0) return VP_OK;
    if ((size_t)ncand > kcap) return vp_fail(ctx, VP_ERR_HIP, "good features: candidate count above its bound");
    u64* d_sorted = nullptr;
    VP_TRY(vpk_hough_sort_keys(ctx, d_k0, d_k1, kcap, d_cnt + 1, 1, ncand, &d_sorted));
    // without a distance to keep (two pixels are at least 1 apart) the first max_corners are the answer: only they come back
    const bool spaced = min_distance * min_distance > 1.0;
    const size_t nback = (!spaced && max_corners > 0) ? std::min<size_t>(ncand, (size_t)max_corners) : ncand;
    u64* hk = (u64*)vp_hstage(ctx, nback * 8);
    if (!hk) return vp_fail(ctx, VP_ERR_NOMEM, "pinned staging");
    VP_TRY(d2h(ctx, hk, d_sorted, nback * 8));
    VP_TRY(vp_synchronize(ctx));
    *n_corners = (int)vp_good_features_select(hk, (long long)nback, w, h, max_corners, min_distance, corners, capacity);
    return VP_OK;
}

extern "C" {

int vp_corner_response_u8(vp_ctx* ctx, const uint8_t* src, size_t stride, int w, int h, int block_size, int ksize, int harris, double k, int border,
                          float* dst)
{
    if (!src || !dst) return vp_fail(ctx, VP_ERR_INVALID, "vp_corner_response_u8: a pointer is missing");
    if (const char* why = vp_corner_response_refusal(w, h, stride, block_size, ksize, k, border)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    const size_t npx = (size_t)w * h;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, npx);
    float* d_dst; W.want(&d_dst, npx * 4);
    VP_TRY(vp_ws_commit(ctx, W, "vp_corner_response_u8"));
    VP_TRY(h2d_rows(ctx, d_src, (size_t)w, src, stride, (size_t)w, h));
    VP_TRY(vpk_corner_response(ctx, d_src, (size_t)w, w, h, block_size, harris != 0, k, border, d_dst));
    VP_TRY(d2h(ctx, dst, d_dst, npx * 4));
    return vp_synchronize(ctx);
}

int vp_corner_response_dev(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int block_size, int ksize, int harris, double k, int border,
                           float* d_dst)
{
    if (!d_src || !d_dst) return vp_fail(ctx, VP_ERR_INVALID, "vp_corner_response_dev: a pointer is missing");
    if (const char* why = vp_corner_response_refusal(w, h, stride, block_size, ksize, k, border)) return vp_fail(ctx, VP_ERR_INVALID, why);
    if ((uintptr_t)d_dst % 4 || dev_overlap(d_src, strided_bytes(stride, (size_t)w, h), d_dst, (size_t)w * h * 4))
        return vp_fail(ctx, VP_ERR_INVALID, "vp_corner_response_dev: dst is not aligned to a float, or overlaps src");
    VP_TRY(check_ctx(ctx));
    return vpk_corner_response(ctx, d_src, stride, w, h, block_size, harris != 0, k, border, d_dst);
}

int vp_good_features_u8(vp_ctx* ctx, const uint8_t* src, size_t stride, int w, int h, int max_corners, double quality_level, double min_distance,
                        const uint8_t* mask, size_t mask_stride, int mask_w, int mask_h, int block_size, int harris, double k, float* corners,
                        int capacity, int* n_corners)
{
    if (!src || !n_corners || (capacity > 0 && !corners)) return vp_fail(ctx, VP_ERR_INVALID, "vp_good_features_u8: a pointer is missing");
    if (const char* why = vp_good_features_refusal(w, h, stride, quality_level, min_distance, mask != nullptr, mask_w, mask_h, mask_stride, block_size, k, capacity))
        return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    const size_t npx = (size_t)w * h;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, npx);
    uint8_t* d_mask = nullptr;
    if (mask) W.want(&d_mask, npx);
    gf_bufs b;
    gf_want(W, w, h, &b);
    VP_TRY(vp_ws_commit(ctx, W, "vp_good_features_u8"));
    VP_TRY(h2d_rows(ctx, d_src, (size_t)w, src, stride, (size_t)w, h));
    if (mask) VP_TRY(h2d_rows(ctx, d_mask, (size_t)w, mask, mask_stride, (size_t)w, h));
    return good_features_run(ctx, d_src, (size_t)w, w, h, max_corners, quality_level, min_distance, d_mask, (size_t)w, nullptr, block_size, harris != 0, k,
                             corners, capacity, n_corners, b);
}

int vp_good_features_dev(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int max_corners, double quality_level, double min_distance,
                         const uint8_t* d_mask, size_t mask_stride, int mask_w, int mask_h, const unsigned long long* d_mask_bits, int block_size,
                         int harris, double k, float* corners, int capacity, int* n_corners)
{
    if (!d_src || !n_corners || (capacity > 0 && !corners)) return vp_fail(ctx, VP_ERR_INVALID, "vp_good_features_dev: a pointer is missing");
    if (d_mask_bits && (uintptr_t)d_mask_bits % 8) return vp_fail(ctx, VP_ERR_INVALID, "vp_good_features_dev: the bit plane must be 8-byte aligned");
    const int has_mask = d_mask != nullptr || d_mask_bits != nullptr;
    if (const char* why = vp_good_features_refusal(w, h, stride, quality_level, min_distance, has_mask, mask_w, mask_h, d_mask ? mask_stride : (size_t)w,
                                                   block_size, k, capacity))
        return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    vp_ws_frame W;
    gf_bufs b;
    gf_want(W, w, h, &b);
    VP_TRY(vp_ws_commit(ctx, W, "vp_good_features_dev"));
    return good_features_run(ctx, d_src, stride, w, h, max_corners, quality_level, min_distance, d_mask_bits ? nullptr : d_mask, mask_stride,
                             reinterpret_cast<const u64*>(d_mask_bits), block_size, harris != 0, k, corners, capacity, n_corners, b);
}

}  // extern "C"
