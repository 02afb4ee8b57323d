// C ABI of libvp.so, colour-histogram tracking: cv2.calcHist, cv2.calcBackProject and cv2.meanShift on host and device images (kernels:
// vp_hist.hip; checks, bin tables, limits and grids: vp_hist_plan.h).
#include "vp_api_util.h"
#include "vp_hist_plan.h"

// what the histogram and the back-projection entries share: pointers of the description, then the description itself
static const char* describe_refusal(int w, int h, int cn, size_t stride, int dims, const int32_t* channels, const int32_t* hist_size, const double* ranges)
{
    if (!channels || !hist_size || !ranges) return "hist: a pointer is missing";
    return vp_hist_refusal(w, h, cn, stride, dims, channels, hist_size, ranges);
}

static size_t hist_total(int dims, const int32_t* hist_size)
{
    size_t t = 1;
    for (int d = 0; d < dims; d++) t *= (size_t)hist_size[d];
    return t;
}

// saturate_u8(round_half_even(double(v) * scale)), as k_bp_fold
static inline uint8_t fold_one(float v, double scale)
{
    const double r = nearbyint((double)v * scale);
    return !(r > 0.0) ? (uint8_t)0 : r >= 255.0 ? (uint8_t)255 : (uint8_t)(int)r;
}

extern "C" {

int vp_calc_hist_u8(vp_ctx* ctx, const uint8_t* src, int w, int h, int cn, int dims, const int32_t* channels, const int32_t* hist_size, const double* ranges,
                    const uint8_t* mask, int mask_w, int mask_h, float* hist)
{
    if (!src || !hist) return vp_fail(ctx, VP_ERR_INVALID, "vp_calc_hist_u8: a pointer is missing");
    const size_t row = w > 0 && cn > 0 ? (size_t)w * cn : 0;
    if (const char* why = describe_refusal(w, h, cn, row, dims, channels, hist_size, ranges)) return vp_fail(ctx, VP_ERR_INVALID, why);
    if (mask)
        if (const char* why = vp_hist_mask_refusal(w, h, mask_w, mask_h, (size_t)mask_w)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    vp_hist_plan P;
    vp_hist_make_plan(w, h, cn, dims, channels, hist_size, ranges, 0, &P);
    const size_t pitch = (row + 3) / 4 * 4, cbytes = (size_t)P.total * 4;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, pitch * h);
    u32* d_cnt; W.want(&d_cnt, cbytes);
    uint8_t* d_mask = nullptr;
    if (mask) W.want(&d_mask, (size_t)w * h);
    VP_TRY(vp_ws_commit(ctx, W, "vp_calc_hist_u8"));
    VP_TRY(h2d_rows(ctx, d_src, pitch, src, row, row, h));
    if (mask) VP_TRY(h2d(ctx, d_mask, mask, (size_t)w * h));
    VP_TRY(vpk_calc_hist(ctx, d_src, pitch, w, h, P, d_mask, (size_t)w, nullptr, d_cnt));
    std::vector<u32> cnt((size_t)P.total);
    VP_TRY(d2h(ctx, cnt.data(), d_cnt, cbytes));
    VP_TRY(vp_synchronize(ctx));
    for (int i = 0; i < P.total; i++) hist[i] = (float)cnt[i];      // exact: a count is at most 2^24
    return VP_OK;
}

int vp_calc_hist_dev(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int cn, int dims, const int32_t* channels, const int32_t* hist_size,
                     const double* ranges, const uint8_t* d_mask, size_t mask_stride, int mask_w, int mask_h, const unsigned long long* d_mask_bits,
                     uint32_t* d_counts, uint32_t* counts_host)
{
    if (!d_src || (!d_counts && !counts_host)) return vp_fail(ctx, VP_ERR_INVALID, "vp_calc_hist_dev: a pointer is missing");
    if (const char* why = describe_refusal(w, h, cn, stride, dims, channels, hist_size, ranges)) return vp_fail(ctx, VP_ERR_INVALID, why);
    if (d_mask || d_mask_bits)
        if (const char* why = vp_hist_mask_refusal(w, h, mask_w, mask_h, d_mask ? mask_stride : (size_t)w)) return vp_fail(ctx, VP_ERR_INVALID, why);
    if (d_mask_bits && (uintptr_t)d_mask_bits % 8) return vp_fail(ctx, VP_ERR_INVALID, "vp_calc_hist_dev: the bit plane must be 8-byte aligned");
    const size_t cbytes = hist_total(dims, hist_size) * 4;
    if (d_counts && ((uintptr_t)d_counts % 4 || dev_overlap(d_src, strided_bytes(stride, (size_t)w * cn, h), d_counts, cbytes)))
        return vp_fail(ctx, VP_ERR_INVALID, "vp_calc_hist_dev: the counters are not 4-byte aligned, or overlap the image");
    VP_TRY(check_ctx(ctx));
    vp_hist_plan P;
    vp_hist_make_plan(w, h, cn, dims, channels, hist_size, ranges, 0, &P);
    u32* d_cnt = d_counts;
    if (!d_cnt) {
        vp_ws_frame W;
        W.want(&d_cnt, cbytes);
        VP_TRY(vp_ws_commit(ctx, W, "vp_calc_hist_dev"));
    }
    VP_TRY(vpk_calc_hist(ctx, d_src, stride, w, h, P, d_mask_bits ? nullptr : d_mask, mask_stride, reinterpret_cast<const u64*>(d_mask_bits), d_cnt));
    if (!counts_host) return VP_OK;
    VP_TRY(d2h(ctx, counts_host, d_cnt, cbytes));
    return vp_synchronize(ctx);
}

int vp_back_project_u8(vp_ctx* ctx, const uint8_t* src, int w, int h, int cn, int dims, const int32_t* channels, const int32_t* hist_size, const double* ranges,
                       const float* hist, double scale, uint8_t* dst)
{
    if (!src || !hist || !dst) return vp_fail(ctx, VP_ERR_INVALID, "vp_back_project_u8: a pointer is missing");
    const size_t row = w > 0 && cn > 0 ? (size_t)w * cn : 0;
    if (const char* why = describe_refusal(w, h, cn, row, dims, channels, hist_size, ranges)) return vp_fail(ctx, VP_ERR_INVALID, why);
    if (!std::isfinite(scale)) return vp_fail(ctx, VP_ERR_INVALID, "back projection: the scale must be finite");
    VP_TRY(check_ctx(ctx));
    vp_hist_plan P;
    vp_hist_make_plan(w, h, cn, dims, channels, hist_size, ranges, 1, &P);
    const size_t pitch = (row + 3) / 4 * 4, dpitch = ((size_t)w + 3) / 4 * 4;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, pitch * h);
    uint8_t* d_dst; W.want(&d_dst, dpitch * h);
    uint8_t* d_table; W.want(&d_table, (size_t)P.total);
    VP_TRY(vp_ws_commit(ctx, W, "vp_back_project_u8"));
    std::vector<uint8_t> table((size_t)P.total);      // the fold, on the host: the histogram is here
    for (int i = 0; i < P.total; i++) table[i] = fold_one(hist[i], scale);
    VP_TRY(h2d_rows(ctx, d_src, pitch, src, row, row, h));
    VP_TRY(h2d(ctx, d_table, table.data(), (size_t)P.total));
    VP_TRY(vpk_back_project(ctx, d_src, pitch, w, h, P, d_table, d_dst, dpitch));
    VP_HIP(ctx, hipMemcpy2DAsync(dst, (size_t)w, d_dst, dpitch, (size_t)w, h, hipMemcpyDeviceToHost, ctx->stream));
    return vp_synchronize(ctx);
}

static const char* bp_dev_refusal(const uint8_t* d_src, size_t stride, int w, int h, int cn, const void* d_from, size_t from_bytes, const uint8_t* d_dst, size_t dst_stride)
{
    if (dst_stride < (size_t)w) return "back projection: the result's stride is below the row";
    const size_t dbytes = strided_bytes(dst_stride, (size_t)w, h);
    if (dev_overlap(d_src, strided_bytes(stride, (size_t)w * cn, h), d_dst, dbytes)) return "back projection: the result overlaps the image";
    if (dev_overlap(d_from, from_bytes, d_dst, dbytes)) return "back projection: the result overlaps the histogram or the table";
    return nullptr;
}

int vp_back_project_dev(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int cn, int dims, const int32_t* channels, const int32_t* hist_size,
                        const double* ranges, const float* d_hist, double scale, uint8_t* d_dst, size_t dst_stride)
{
    if (!d_src || !d_hist || !d_dst) return vp_fail(ctx, VP_ERR_INVALID, "vp_back_project_dev: a pointer is missing");
    if (const char* why = describe_refusal(w, h, cn, stride, dims, channels, hist_size, ranges)) return vp_fail(ctx, VP_ERR_INVALID, why);
    if (!std::isfinite(scale)) return vp_fail(ctx, VP_ERR_INVALID, "back projection: the scale must be finite");
    if ((uintptr_t)d_hist % 4) return vp_fail(ctx, VP_ERR_INVALID, "back projection: the histogram is not 4-byte aligned");
    const size_t total = hist_total(dims, hist_size);
    if (const char* why = bp_dev_refusal(d_src, stride, w, h, cn, d_hist, total * 4, d_dst, dst_stride)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    vp_hist_plan P;
    vp_hist_make_plan(w, h, cn, dims, channels, hist_size, ranges, 1, &P);
    vp_ws_frame W;
    uint8_t* d_table; W.want(&d_table, total);
    VP_TRY(vp_ws_commit(ctx, W, "vp_back_project_dev"));
    VP_TRY(vpk_back_project_fold(ctx, d_hist, P.total, scale, d_table));
    return vpk_back_project(ctx, d_src, stride, w, h, P, d_table, d_dst, dst_stride);
}

int vp_back_project_table_dev(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int cn, int dims, const int32_t* channels, const int32_t* hist_size,
                              const double* ranges, const uint8_t* d_table, uint8_t* d_dst, size_t dst_stride)
{
    if (!d_src || !d_table || !d_dst) return vp_fail(ctx, VP_ERR_INVALID, "vp_back_project_table_dev: a pointer is missing");
    if (const char* why = describe_refusal(w, h, cn, stride, dims, channels, hist_size, ranges)) return vp_fail(ctx, VP_ERR_INVALID, why);
    if (const char* why = bp_dev_refusal(d_src, stride, w, h, cn, d_table, hist_total(dims, hist_size), d_dst, dst_stride)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    vp_hist_plan P;
    vp_hist_make_plan(w, h, cn, dims, channels, hist_size, ranges, 1, &P);
    return vpk_back_project(ctx, d_src, stride, w, h, P, d_table, d_dst, dst_stride);
}

int vp_mean_shift_dev(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, const int32_t* windows, int n, int max_iter, double eps, int32_t* d_out,
                      int32_t* out_host)
{
    if (!d_src || !windows || (!d_out && !out_host)) return vp_fail(ctx, VP_ERR_INVALID, "vp_mean_shift_dev: a pointer is missing");
    if (const char* why = vp_mean_shift_refusal(w, h, stride, windows, n)) return vp_fail(ctx, VP_ERR_INVALID, why);
    if (max_iter > HS_MS_MAX_ITER) return vp_fail(ctx, VP_ERR_UNSUPPORTED, "mean shift: more than 100000 iterations");
    const size_t obytes = (size_t)n * 5 * 4, wbytes = (size_t)n * 4 * 4;
    if (d_out && ((uintptr_t)d_out % 4 || dev_overlap(d_src, strided_bytes(stride, (size_t)w, h), d_out, obytes)))
        return vp_fail(ctx, VP_ERR_INVALID, "vp_mean_shift_dev: the result is not 4-byte aligned, or overlaps the image");
    VP_TRY(check_ctx(ctx));
    vp_ws_frame W;
    int32_t* d_win; W.want(&d_win, wbytes);
    int32_t* d_res = d_out;
    if (!d_res) W.want(&d_res, obytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_mean_shift_dev"));
    // the windows go over in a pinned chunk of the context's ring: the copy is enqueued, nothing waits for it
    int slot = -1;
    uint8_t* hp = vp_ring_take(ctx, wbytes, &slot);
    if (!hp) return vp_fail(ctx, VP_ERR_NOMEM, "pinned staging");
    memcpy(hp, windows, wbytes);
    int rc = h2d(ctx, d_win, hp, wbytes);
    if (rc == VP_OK) rc = vpk_mean_shift(ctx, d_src, stride, w, h, d_win, n, vp_ms_iters(max_iter), vp_ms_eps2(eps), d_res);
    vp_ring_done(ctx, slot);
    if (rc != VP_OK || !out_host) return rc;
    VP_TRY(d2h(ctx, out_host, d_res, obytes));
    return vp_synchronize(ctx);
}

}  // extern "C"
