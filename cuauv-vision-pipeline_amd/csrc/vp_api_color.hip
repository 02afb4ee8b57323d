// C ABI of libvp.so, colour family: conversions, in-range tests, colour distance, colour balance and white balance (kernels:
// vp_color / vp_balance / vp_whitebal).  Host forms stage their operands and synchronise; device forms only enqueue.
#include "vp_api_util.h"

extern "C" {

int vp_cvt_color_u8(vp_ctx* ctx, int code, const uint8_t* src, size_t src_stride, int w, int h, uint8_t* dst_i,
                    uint8_t* const* planes)
{
    VP_TRY(check_ctx(ctx));
    if (!src || w <= 0 || h <= 0 || h > 65535) return vp_fail(ctx, VP_ERR_INVALID, "vp_cvt_color_u8 arguments");
    int scn = 0, dcn = 0;
    if (!vp_cvt_channels(code, &scn, &dcn)) return vp_fail(ctx, VP_ERR_INVALID, "conversion code");
    if (src_stride < (size_t)w * scn) return vp_fail(ctx, VP_ERR_INVALID, "src_stride");
    if (planes && dcn != 3 && code != VP_BGR2GRAY) return vp_fail(ctx, VP_ERR_INVALID, "split planes of a 1- or 4-channel result");
    const size_t npx = (size_t)w * h;
    uint8_t* hp[3] = {nullptr, nullptr, nullptr};
    if (planes)
        for (int c = 0; c < dcn; c++) hp[c] = planes[c];
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, npx * scn);
    uint8_t* d_dst; W.want(&d_dst, npx * dcn);
    uint8_t* dp[3] = {nullptr, nullptr, nullptr};
    for (int c = 0; c < 3; c++)
        if (hp[c]) W.want(&dp[c], npx);
    VP_TRY(vp_ws_commit(ctx, W, "vp_cvt_color_u8"));
    VP_TRY(h2d_rows(ctx, d_src, (size_t)w * scn, src, src_stride, (size_t)w * scn, h));
    if (code == VP_HSV2BGR) {
        if (planes) return vp_fail(ctx, VP_ERR_UNSUPPORTED, "HSV2BGR: split planes");
        VP_TRY(vpk_hsv2bgr(ctx, d_src, npx, d_dst));
    } else {
        VP_TRY(vpk_cvt_color(ctx, code, d_src, (size_t)w * scn, w, h, dst_i ? d_dst : nullptr, dp[0], dp[1], dp[2]));
    }
    if (dst_i) VP_TRY(d2h(ctx, dst_i, d_dst, npx * dcn));
    for (int c = 0; c < 3; c++)
        if (hp[c]) VP_TRY(d2h(ctx, hp[c], dp[c], npx));
    return vp_synchronize(ctx);
}

int vp_color_balance_u8(vp_ctx* ctx, const uint8_t* src, int w, int h, int flags, int hblocks, int vblocks, uint8_t* dst)
{
    VP_TRY(check_ctx(ctx));
    if (!src || !dst || w <= 0 || h <= 0 || hblocks <= 0 || vblocks <= 0) return vp_fail(ctx, VP_ERR_INVALID, "vp_color_balance_u8 arguments");
    const size_t npx = (size_t)w * h;
    const size_t tiles = (flags & VP_CB_EQUALIZE_RGB) ? (size_t)hblocks * vblocks : 1;
    if (tiles > 1024) return vp_fail(ctx, VP_ERR_UNSUPPORTED, "colour balance: too many tiles");
    vp_ws_frame W;
    uint8_t* d_img; W.want(&d_img, npx * 3);
    vp_balance_ws bw;
    vp_balance_want(W, 1, (int)tiles, flags, &bw);
    VP_TRY(vp_ws_commit(ctx, W, "vp_color_balance_u8"));
    VP_TRY(h2d(ctx, d_img, src, npx * 3));
    VP_TRY(vpk_color_balance(ctx, d_img, d_img, w, h, 1, flags, hblocks, vblocks, bw));
    VP_TRY(d2h(ctx, dst, d_img, npx * 3));
    return vp_synchronize(ctx);
}

int vp_color_balance_last_folds(vp_ctx* ctx, int32_t* tiles_folded)
{
    VP_TRY(check_ctx(ctx));
    if (!tiles_folded) return vp_fail(ctx, VP_ERR_INVALID, "vp_color_balance_last_folds arguments");
    *tiles_folded = 0;
    if (!ctx->cb.folds_dev) return VP_OK;
    uint32_t v = 0;
    VP_HIP(ctx, hipMemcpyAsync(&v, ctx->cb.folds_dev, 4, hipMemcpyDeviceToHost, ctx->stream));
    VP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *tiles_folded = (int32_t)v;
    return VP_OK;
}

int vp_color_balance_dev(vp_ctx* ctx, const uint8_t* src, uint8_t* dst, int w, int h, int n, int flags, int hblocks, int vblocks)
{
    VP_TRY(check_ctx(ctx));
    if (!src || !dst || w <= 0 || h <= 0 || n <= 0 || hblocks <= 0 || vblocks <= 0) return vp_fail(ctx, VP_ERR_INVALID, "vp_color_balance_dev arguments");
    const size_t tiles = (flags & VP_CB_EQUALIZE_RGB) ? (size_t)hblocks * vblocks : 1;
    if (tiles > 1024) return vp_fail(ctx, VP_ERR_UNSUPPORTED, "colour balance: too many tiles");
    vp_ws_frame W;
    vp_balance_ws bw;
    vp_balance_want(W, n, (int)tiles, flags, &bw);
    VP_TRY(vp_ws_commit(ctx, W, "vp_color_balance_dev"));
    return vpk_color_balance(ctx, src, dst, w, h, n, flags, hblocks, vblocks, bw);
}

int vp_cvt_bgr2lab_f32(vp_ctx* ctx, const float* src, int w, int h, float* dst)
{
    VP_TRY(check_ctx(ctx));
    if (!src || !dst || w <= 0 || h <= 0) return vp_fail(ctx, VP_ERR_INVALID, "vp_cvt_bgr2lab_f32 arguments");
    const size_t npx = (size_t)w * h;
    vp_ws_frame W;
    float* d_src; W.want(&d_src, npx * 12);
    float* d_dst; W.want(&d_dst, npx * 12);
    VP_TRY(vp_ws_commit(ctx, W, "vp_cvt_bgr2lab_f32"));
    VP_TRY(h2d(ctx, d_src, src, npx * 12));
    VP_TRY(vpk_bgr2lab_f32(ctx, d_src, npx, d_dst));
    VP_TRY(d2h(ctx, dst, d_dst, npx * 12));
    return vp_synchronize(ctx);
}

int vp_order_stats_f32(vp_ctx* ctx, const float* src, size_t n, size_t k, float* v_k, float* v_k1)
{
    VP_TRY(check_ctx(ctx));
    if (!src || !v_k || n == 0 || k >= n) return vp_fail(ctx, VP_ERR_INVALID, "vp_order_stats_f32 arguments");
    vp_ws_frame W;
    float* d_src; W.want(&d_src, n * 4);
    u32* d_hist; W.want(&d_hist, 1024);
    VP_TRY(vp_ws_commit(ctx, W, "vp_order_stats_f32"));
    VP_TRY(h2d(ctx, d_src, src, n * 4));
    VP_TRY(vpk_kth_f32(ctx, d_src, n, k, d_hist, v_k));
    if (v_k1) VP_TRY(vpk_kth_f32(ctx, d_src, n, k + 1 < n ? k + 1 : n - 1, d_hist, v_k1));
    return VP_OK;
}

int vp_inrange_u8(vp_ctx* ctx, const uint8_t* src, size_t src_stride, int w, int h, int cn, const int32_t* lo, const int32_t* hi,
                  uint8_t* dst)
{
    VP_TRY(check_ctx(ctx));
    if (!src || !dst || !lo || !hi || w <= 0 || h <= 0 || h > 65535 || (cn != 1 && cn != 3) || src_stride < (size_t)w * cn)
        return vp_fail(ctx, VP_ERR_INVALID, "vp_inrange_u8 arguments");
    vp_range3 q;
    norm_range(cn, lo, hi, &q);
    const size_t npx = (size_t)w * h;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, npx * cn);
    uint8_t* d_dst; W.want(&d_dst, npx);
    VP_TRY(vp_ws_commit(ctx, W, "vp_inrange_u8"));
    VP_TRY(h2d_rows(ctx, d_src, (size_t)w * cn, src, src_stride, (size_t)w * cn, h));
    VP_TRY(vpk_inrange_u8(ctx, d_src, (size_t)w * cn, w, h, cn, q, d_dst));
    VP_TRY(d2h(ctx, dst, d_dst, npx));
    return vp_synchronize(ctx);
}

int vp_inrange_f32(vp_ctx* ctx, const float* src, size_t src_stride_bytes, int w, int h, float lo, float hi, uint8_t* dst)
{
    VP_TRY(check_ctx(ctx));
    if (!src || !dst || w <= 0 || h <= 0 || h > 65535 || src_stride_bytes < (size_t)w * 4)
        return vp_fail(ctx, VP_ERR_INVALID, "vp_inrange_f32 arguments");
    const size_t npx = (size_t)w * h;
    vp_ws_frame W;
    float* d_src; W.want(&d_src, npx * 4);
    uint8_t* d_dst; W.want(&d_dst, npx);
    VP_TRY(vp_ws_commit(ctx, W, "vp_inrange_f32"));
    VP_TRY(h2d_rows(ctx, d_src, (size_t)w * 4, src, src_stride_bytes, (size_t)w * 4, h));
    VP_TRY(vpk_inrange_f32(ctx, d_src, (size_t)w * 4, w, h, lo, hi, d_dst));
    VP_TRY(d2h(ctx, dst, d_dst, npx));
    return vp_synchronize(ctx);
}

int vp_color_distance_u8(vp_ctx* ctx, const uint8_t* const* planes, int w, int h, const float* color, const float* wts, int skipmask,
                         float* dist2_out, uint8_t* sqrt_out)
{
    VP_TRY(check_ctx(ctx));
    if (!planes || !color || !wts || w <= 0 || h <= 0) return vp_fail(ctx, VP_ERR_INVALID, "vp_color_distance_u8 arguments");
    for (int c = 0; c < 3; c++)
        if (!(skipmask & (1 << c)) && !planes[c]) return vp_fail(ctx, VP_ERR_INVALID, "missing plane");
    const size_t npx = (size_t)w * h;
    vp_ws_frame W;
    uint8_t* dp[3] = {nullptr, nullptr, nullptr};
    for (int c = 0; c < 3; c++)
        if (!(skipmask & (1 << c))) W.want(&dp[c], npx);
    float* d_d2; W.want(&d_d2, npx * 4);
    uint8_t* d_sq; W.want(&d_sq, npx);
    VP_TRY(vp_ws_commit(ctx, W, "vp_color_distance_u8"));
    for (int c = 0; c < 3; c++)
        if (dp[c]) VP_TRY(h2d(ctx, dp[c], planes[c], npx));
    VP_TRY(vpk_color_distance(ctx, dp[0], dp[1], dp[2], npx, color, wts, skipmask, d_d2, d_sq));
    if (dist2_out) VP_TRY(d2h(ctx, dist2_out, d_d2, npx * 4));
    if (sqrt_out) VP_TRY(d2h(ctx, sqrt_out, d_sq, npx));
    return vp_synchronize(ctx);
}

// ---- device-resident forms of the per-operator entry points ---------------------------------------------------------------------
// Same arithmetic, same argument meaning; images are device pointers (packed rows unless a stride is taken), nothing is copied
// and nothing is synchronised: the call enqueues on the context's stream and returns.  They let the Python mirror keep the
// intermediate images of a module's process() in HBM between operator calls (modules/red_buoy.py:21-38: the Lab image, its
// planes, the threshold mask and both cleaned masks never need to visit the host).

int vp_cvt_color_dev(vp_ctx* ctx, int code, const uint8_t* d_src, size_t src_stride, int w, int h, uint8_t* d_dst, uint8_t* const* d_planes)
{
    VP_TRY(check_ctx(ctx));
    if (!d_src || w <= 0 || h <= 0 || h > 65535) return vp_fail(ctx, VP_ERR_INVALID, "vp_cvt_color_dev arguments");
    int scn = 0, dcn = 0;
    if (!vp_cvt_channels(code, &scn, &dcn)) return vp_fail(ctx, VP_ERR_INVALID, "conversion code");
    if (src_stride < (size_t)w * scn) return vp_fail(ctx, VP_ERR_INVALID, "src_stride");
    if (d_planes && dcn != 3 && code != VP_BGR2GRAY) return vp_fail(ctx, VP_ERR_INVALID, "split planes of a 1- or 4-channel result");
    uint8_t* dp[3] = {nullptr, nullptr, nullptr};
    if (d_planes)
        for (int c = 0; c < dcn; c++) dp[c] = d_planes[c];
    if (code == VP_HSV2BGR) {
        if (d_planes || !d_dst || src_stride != (size_t)w * 3) return vp_fail(ctx, VP_ERR_UNSUPPORTED, "HSV2BGR: packed rows, no split planes");
        return vpk_hsv2bgr(ctx, d_src, (size_t)w * h, d_dst);
    }
    return vpk_cvt_color(ctx, code, d_src, src_stride, w, h, d_dst, dp[0], dp[1], dp[2]);
}

int vp_inrange_u8_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, int cn, const int32_t* lo, const int32_t* hi, uint8_t* d_dst)
{
    VP_TRY(check_ctx(ctx));
    if (!d_src || !d_dst || !lo || !hi || w <= 0 || h <= 0 || h > 65535 || (cn != 1 && cn != 3) || src_stride < (size_t)w * cn)
        return vp_fail(ctx, VP_ERR_INVALID, "vp_inrange_u8_dev arguments");
    vp_range3 q;
    norm_range(cn, lo, hi, &q);
    return vpk_inrange_u8(ctx, d_src, src_stride, w, h, cn, q, d_dst);
}

int vp_inrange_u8_bits_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, int cn, const int32_t* lo, const int32_t* hi, uint8_t* d_dst,
                           unsigned long long* d_bits, int* made_bits)
{
    VP_TRY(check_ctx(ctx));
    if (!d_src || !d_dst || !lo || !hi || w <= 0 || h <= 0 || h > 65535 || (cn != 1 && cn != 3) || src_stride < (size_t)w * cn)
        return vp_fail(ctx, VP_ERR_INVALID, "vp_inrange_u8_bits_dev arguments");
    vp_range3 q;
    norm_range(cn, lo, hi, &q);
    return vpk_inrange_u8(ctx, d_src, src_stride, w, h, cn, q, d_dst, reinterpret_cast<u64*>(d_bits), made_bits);
}

static int wb_args(vp_ctx* ctx, const void* src, size_t src_stride, int w, int h, int kernel_size, const void* dst)
{
    if (!src || !dst || w <= 0 || h <= 0 || h > 65535 || src_stride < (size_t)w * 3) return vp_fail(ctx, VP_ERR_INVALID, "white balance arguments");
    if (kernel_size != VP_WB_GLOBAL_MEAN && (kernel_size < 1 || kernel_size % 2 == 0)) return vp_fail(ctx, VP_ERR_INVALID, "white balance: kernel size must be odd");
    if (kernel_size > VP_WB_MAX_KERNEL) return vp_fail(ctx, VP_ERR_UNSUPPORTED, "white balance: kernel size above VP_WB_MAX_KERNEL");
    return VP_OK;
}

// the means go through the workspace and come back only when asked for; the device forms stay asynchronous otherwise
struct wb_bufs { float* mean; vp_whitebal_ws k; };
static void wb_want(vp_ws_frame& W, int w, int h, int kernel_size, wb_bufs* b)
{
    W.want(&b->mean, 8);
    vp_white_balance_want(W, w, h, kernel_size, &b->k);
}
static int wb_run(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int kernel_size, uint8_t* d_dst, float* ab_mean_out, const wb_bufs& b)
{
    VP_TRY(vpk_white_balance(ctx, d_src, stride, w, h, kernel_size, d_dst, b.mean, b.k));
    if (ab_mean_out && kernel_size == VP_WB_GLOBAL_MEAN) {
        VP_TRY(d2h(ctx, ab_mean_out, b.mean, 8));
        return vp_synchronize(ctx);
    }
    return VP_OK;
}

int vp_white_balance_u8(vp_ctx* ctx, const uint8_t* src, size_t src_stride, int w, int h, int kernel_size, uint8_t* dst, float* ab_mean_out)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(wb_args(ctx, src, src_stride, w, h, kernel_size, dst));
    const size_t npx = (size_t)w * h;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, npx * 3);
    uint8_t* d_dst; W.want(&d_dst, npx * 3);
    wb_bufs b;
    wb_want(W, w, h, kernel_size, &b);
    VP_TRY(vp_ws_commit(ctx, W, "vp_white_balance_u8"));
    VP_TRY(h2d_rows(ctx, d_src, (size_t)w * 3, src, src_stride, (size_t)w * 3, h));
    VP_TRY(wb_run(ctx, d_src, (size_t)w * 3, w, h, kernel_size, d_dst, ab_mean_out, b));
    VP_TRY(d2h(ctx, dst, d_dst, npx * 3));
    return vp_synchronize(ctx);
}

int vp_white_balance_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, int kernel_size, uint8_t* d_dst, float* ab_mean_out)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(wb_args(ctx, d_src, src_stride, w, h, kernel_size, d_dst));
    vp_ws_frame W;
    wb_bufs b;
    wb_want(W, w, h, kernel_size, &b);
    VP_TRY(vp_ws_commit(ctx, W, "vp_white_balance_dev"));
    return wb_run(ctx, d_src, src_stride, w, h, kernel_size, d_dst, ab_mean_out, b);
}

}  // extern "C"
