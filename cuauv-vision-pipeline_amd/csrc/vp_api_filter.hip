// C ABI of libvp.so, filters: thresholds, Otsu and histogram, blur, resize, warp, adaptive thresholds, Canny, Hough lines and
// circles, letterbox, NMS and the element-wise operators (kernels: vp_filter / vp_adaptive / vp_hough* / vp_yolo / vp_elementwise).
// Host forms stage their operands and synchronise; device forms take the image where the operator before them left it, copy nothing
// and only enqueue (the histogram and the counters bring numbers back and synchronise for them).  Each host / device pair shares
// one *_args check, which also normalises the parameters; what differs between the forms stays in the entry.
#include "vp_api_util.h"
#include "vp_deriv_plan.h"
#include "vp_clahe_plan.h"
#include "vp_remap_plan.h"
#include "vp_box_plan.h"
#include <mutex>

extern "C" {

// cv2.threshold on 8-bit images: the threshold floored into [-1, 256], maxval rounded into [0, 255]
static int thresh_args(vp_ctx* ctx, const char* who, const void* src, const void* dst, size_t n, double thresh, double maxval, int type, int* ithresh,
                       int* imaxval)
{
    if (!src || !dst || n == 0 || type < VP_THRESH_BINARY || type > VP_THRESH_TOZERO_INV || thresh != thresh || maxval != maxval)
        return vp_fail(ctx, VP_ERR_INVALID, who);
    const double ft = floor(thresh);
    *ithresh = ft < -1 ? -1 : (ft > 256 ? 256 : (int)ft);
    const double rm = nearbyint(maxval);
    *imaxval = rm < 0 ? 0 : (rm > 255 ? 255 : (int)rm);
    return VP_OK;
}

// Otsu: the same without a threshold of the caller's; the histogram counts in 32 bits
static int otsu_args(vp_ctx* ctx, const char* who, const void* src, const void* dst, size_t n, double maxval, int type, int* imaxval)
{
    int ithresh;
    if (n > 0xffffffffull) return vp_fail(ctx, VP_ERR_INVALID, who);
    return thresh_args(ctx, who, src, dst, n, 0.0, maxval, type, &ithresh, imaxval);
}

int vp_threshold_u8(vp_ctx* ctx, const uint8_t* src, size_t n, double thresh, double maxval, int type, uint8_t* dst)
{
    VP_TRY(check_ctx(ctx));
    int ithresh, imaxval;
    VP_TRY(thresh_args(ctx, "vp_threshold_u8 arguments", src, dst, n, thresh, maxval, type, &ithresh, &imaxval));
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, n);
    uint8_t* d_dst; W.want(&d_dst, n);
    VP_TRY(vp_ws_commit(ctx, W, "vp_threshold_u8"));
    VP_TRY(h2d(ctx, d_src, src, n));
    VP_TRY(vpk_threshold_u8(ctx, d_src, n, ithresh, imaxval, type, d_dst));
    VP_TRY(d2h(ctx, dst, d_dst, n));
    return vp_synchronize(ctx);
}

int vp_threshold_u8_dev(vp_ctx* ctx, const uint8_t* d_src, size_t n, double thresh, double maxval, int type, uint8_t* d_dst)
{
    VP_TRY(check_ctx(ctx));
    int ithresh, imaxval;
    VP_TRY(thresh_args(ctx, "vp_threshold_u8_dev arguments", d_src, d_dst, n, thresh, maxval, type, &ithresh, &imaxval));
    if (dev_overlap(d_src, n, d_dst, n)) return vp_fail(ctx, VP_ERR_INVALID, "vp_threshold_u8_dev: dst overlaps src");
    return vpk_threshold_u8(ctx, d_src, n, ithresh, imaxval, type, d_dst);
}

int vp_otsu_threshold_u8(vp_ctx* ctx, const uint8_t* src, size_t n, double maxval, int type, double* thresh_out, uint8_t* dst)
{
    VP_TRY(check_ctx(ctx));
    int imaxval;
    VP_TRY(otsu_args(ctx, "vp_otsu_threshold_u8 arguments", src, dst, n, maxval, type, &imaxval));
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, n);
    uint8_t* d_dst; W.want(&d_dst, n);
    u32* d_hist; W.want(&d_hist, 1024);
    VP_TRY(vp_ws_commit(ctx, W, "vp_otsu_threshold_u8"));
    VP_TRY(h2d(ctx, d_src, src, n));
    VP_TRY(vpk_hist_u8(ctx, d_src, n, d_hist));
    u32 h[256];
    VP_TRY(d2h(ctx, h, d_hist, 1024));
    VP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // imgproc/src/thresh.cpp getThreshVal_Otsu_8u, statement by statement
    const double scale = 1. / (double)n;
    double mu = 0;
    for (int i = 0; i < 256; i++) mu += i * (double)h[i];
    mu *= scale;
    double mu1 = 0, q1 = 0, max_sigma = 0, max_val = 0;
    for (int i = 0; i < 256; i++) {
        const double p_i = h[i] * scale;
        mu1 *= q1;
        q1 += p_i;
        const double q2 = 1. - q1;
        if (std::min(q1, q2) < 1.1920929e-07 || std::max(q1, q2) > 1. - 1.1920929e-07) continue;
        mu1 = (mu1 + i * p_i) / q1;
        const double mu2 = (mu - q1 * mu1) / q2;
        const double sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2);
        if (sigma > max_sigma) { max_sigma = sigma; max_val = i; }
    }
    if (thresh_out) *thresh_out = max_val;
    VP_TRY(vpk_threshold_u8(ctx, d_src, n, (int)max_val, imaxval, type, d_dst));
    VP_TRY(d2h(ctx, dst, d_dst, n));
    return vp_synchronize(ctx);
}

// histogram -> Otsu's scan by one wave -> threshold from the word the scan wrote: three launches, nothing comes back
int vp_otsu_threshold_dev(vp_ctx* ctx, const uint8_t* d_src, size_t n, double maxval, int type, double* d_thresh, uint8_t* d_dst)
{
    VP_TRY(check_ctx(ctx));
    int imaxval;
    VP_TRY(otsu_args(ctx, "vp_otsu_threshold_dev arguments", d_src, d_dst, n, maxval, type, &imaxval));
    if (dev_overlap(d_src, n, d_dst, n)) return vp_fail(ctx, VP_ERR_INVALID, "vp_otsu_threshold_dev: dst overlaps src");
    vp_ws_frame W;
    u32* d_hist; W.want(&d_hist, 1024);
    int32_t* d_it; W.want(&d_it, 4);
    VP_TRY(vp_ws_commit(ctx, W, "vp_otsu_threshold_dev"));
    VP_TRY(vpk_hist_u8(ctx, d_src, n, d_hist));
    VP_TRY(vpk_otsu_scan(ctx, d_hist, n, d_thresh, d_it));
    return vpk_threshold_u8(ctx, d_src, n, 0, imaxval, type, d_dst, d_it);
}

int vp_hist_u8_dev(vp_ctx* ctx, const uint8_t* d_src, size_t n, uint32_t* hist)
{
    VP_TRY(check_ctx(ctx));
    if (!d_src || !hist || n == 0 || n > 0xffffffffull) return vp_fail(ctx, VP_ERR_INVALID, "vp_hist_u8_dev arguments");
    vp_ws_frame W;
    u32* d_hist; W.want(&d_hist, 1024);
    VP_TRY(vp_ws_commit(ctx, W, "vp_hist_u8_dev"));
    VP_TRY(vpk_hist_u8(ctx, d_src, n, d_hist));
    VP_TRY(d2h(ctx, hist, d_hist, 1024));
    return vp_synchronize(ctx);
}

// cv2.equalizeHist and CLAHE on 8-bit single-channel images.  Their checks are pure host arithmetic and come before the context is
// looked at, so a rejected call has touched nothing.  What the device forms add: the stride, and no overlap.
static int plane_args(vp_ctx* ctx, const char* who, const void* src, const void* dst, int w, int h)
{
    if (!src || !dst || w <= 0 || h <= 0) return vp_fail(ctx, VP_ERR_INVALID, who);
    return VP_OK;
}

static int plane_dev_args(vp_ctx* ctx, const char* who, const void* d_src, size_t src_stride, int w, int h, const void* d_dst)
{
    if (src_stride < (size_t)w || dev_overlap(d_src, strided_bytes(src_stride, (size_t)w, h), d_dst, (size_t)w * h)) return vp_fail(ctx, VP_ERR_INVALID, who);
    return VP_OK;
}

static int eqhist_args(vp_ctx* ctx, const char* who, const void* src, const void* dst, int w, int h)
{
    VP_TRY(plane_args(ctx, who, src, dst, w, h));
    if ((long long)w * h > CL_MAX_PIXELS) return vp_fail(ctx, VP_ERR_UNSUPPORTED, who);
    return VP_OK;
}

// the plan is the argument check (vp_clahe_plan.h)
static int clahe_args(vp_ctx* ctx, const char* who, const void* src, const void* dst, int w, int h, double clip_limit, int tiles_x, int tiles_y, vp_clahe_plan* P)
{
    VP_TRY(plane_args(ctx, who, src, dst, w, h));
    *P = vp_clahe_make_plan(w, h, clip_limit, tiles_x, tiles_y, ctx ? ctx->opt.v[VP_OPT_CLAHE_SPLIT] : 0);
    if (P->status == VP_CLAHE_INVALID) return vp_fail(ctx, VP_ERR_INVALID, who);
    if (P->status != VP_CLAHE_OK) return vp_fail(ctx, VP_ERR_UNSUPPORTED, who);
    return VP_OK;
}

int vp_equalize_hist_u8(vp_ctx* ctx, const uint8_t* src, int w, int h, uint8_t* dst)
{
    VP_TRY(eqhist_args(ctx, "vp_equalize_hist_u8 arguments", src, dst, w, h));
    VP_TRY(check_ctx(ctx));
    const size_t n = (size_t)w * h;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, n);
    uint8_t* d_dst; W.want(&d_dst, n);
    u32* d_hist; W.want(&d_hist, 1024);
    uint8_t* d_lut; W.want(&d_lut, 256);
    VP_TRY(vp_ws_commit(ctx, W, "vp_equalize_hist_u8"));
    VP_TRY(h2d(ctx, d_src, src, n));
    VP_TRY(vpk_equalize_hist(ctx, d_src, (size_t)w, w, h, d_hist, d_lut, d_dst));
    VP_TRY(d2h(ctx, dst, d_dst, n));
    return vp_synchronize(ctx);
}

// histogram -> table by one wave -> table applied from device memory: three launches, nothing comes back
int vp_equalize_hist_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, uint8_t* d_dst)
{
    VP_TRY(eqhist_args(ctx, "vp_equalize_hist_dev arguments", d_src, d_dst, w, h));
    VP_TRY(plane_dev_args(ctx, "vp_equalize_hist_dev: src_stride, or dst overlaps src", d_src, src_stride, w, h, d_dst));
    VP_TRY(check_ctx(ctx));
    vp_ws_frame W;
    u32* d_hist; W.want(&d_hist, 1024);
    uint8_t* d_lut; W.want(&d_lut, 256);
    VP_TRY(vp_ws_commit(ctx, W, "vp_equalize_hist_dev"));
    return vpk_equalize_hist(ctx, d_src, src_stride, w, h, d_hist, d_lut, d_dst);
}


int vp_clahe_u8(vp_ctx* ctx, const uint8_t* src, int w, int h, double clip_limit, int tiles_x, int tiles_y, uint8_t* dst)
{
    vp_clahe_plan P;
    VP_TRY(clahe_args(ctx, "vp_clahe_u8 arguments", src, dst, w, h, clip_limit, tiles_x, tiles_y, &P));
    VP_TRY(check_ctx(ctx));
    const size_t n = (size_t)w * h;
    const int tiles = tiles_x * tiles_y;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, n);
    uint8_t* d_dst; W.want(&d_dst, n);
    uint8_t* d_luts; W.want(&d_luts, (size_t)tiles * 256);
    u32* d_part; W.want(&d_part, (size_t)tiles * 1024);
    VP_TRY(vp_ws_commit(ctx, W, "vp_clahe_u8"));
    VP_TRY(h2d(ctx, d_src, src, n));
    VP_TRY(vpk_clahe(ctx, d_src, (size_t)w, w, h, tiles_x, tiles_y, P, d_part, d_luts, d_dst));
    VP_TRY(d2h(ctx, dst, d_dst, n));
    return vp_synchronize(ctx);
}

int vp_clahe_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, double clip_limit, int tiles_x, int tiles_y, uint8_t* d_dst)
{
    vp_clahe_plan P;
    VP_TRY(clahe_args(ctx, "vp_clahe_dev arguments", d_src, d_dst, w, h, clip_limit, tiles_x, tiles_y, &P));
    VP_TRY(plane_dev_args(ctx, "vp_clahe_dev: src_stride, or dst overlaps src", d_src, src_stride, w, h, d_dst));
    VP_TRY(check_ctx(ctx));
    const int tiles = tiles_x * tiles_y;
    vp_ws_frame W;
    uint8_t* d_luts; W.want(&d_luts, (size_t)tiles * 256);
    u32* d_part; W.want(&d_part, (size_t)tiles * 1024);
    VP_TRY(vp_ws_commit(ctx, W, "vp_clahe_dev"));
    return vpk_clahe(ctx, d_src, src_stride, w, h, tiles_x, tiles_y, P, d_part, d_luts, d_dst);
}

// VP_OPT_BLUR_ONEPASS left at its default: the one-pass kernel serves the classes in which it measured faster than the two passes
// on the MI355X by more than the box-to-box spread (tools/exp_dev_ops.py --part blur): three channels, kernels
// up to 21 (1080p: 27 % faster at 3, 9 % at 15, 5 % at 21; 12 % slower at 31).  One channel gains 4 % at 3 and loses from 7 on, and
// two and four channels were not measured: they stay on the two passes.
#define BLUR_ONEPASS_MAX_K 21
static bool blur_onepass_measured_faster(int cn, int kw, int kh) { return cn == 3 && kw <= BLUR_ONEPASS_MAX_K && kh <= BLUR_ONEPASS_MAX_K; }

// cv2.GaussianBlur: odd kernels up to 511; a negative sigma counts as 0 (from the kernel size), sigma2 <= 0 takes sigma1
static int blur_args(vp_ctx* ctx, const char* who, const void* src, const void* dst, int w, int h, int cn, int kw, int kh, double* sigma1, double* sigma2)
{
    if (!src || !dst || w <= 0 || h <= 0 || h > 65535 || cn < 1 || cn > 4 || kw <= 0 || kh <= 0 || !(kw & 1) || !(kh & 1) || kw > 511 || kh > 511)
        return vp_fail(ctx, VP_ERR_INVALID, who);
    if (*sigma1 < 0) *sigma1 = 0;
    if (*sigma2 <= 0) *sigma2 = *sigma1;
    return VP_OK;
}

int vp_gaussian_blur_u8(vp_ctx* ctx, const uint8_t* src, int w, int h, int cn, int kw, int kh, double sigma1, double sigma2, uint8_t* dst)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(blur_args(ctx, "vp_gaussian_blur_u8 arguments", src, dst, w, h, cn, kw, kh, &sigma1, &sigma2));
    const size_t nbytes = (size_t)w * h * cn;
    uint16_t taps[1024];
    vp_gaussian_taps(kw, sigma1, taps);
    vp_gaussian_taps(kh, sigma2, taps + kw);
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, nbytes);
    uint8_t* d_dst; W.want(&d_dst, nbytes);
    uint16_t* d_tmp; W.want(&d_tmp, nbytes * 2);
    uint16_t* d_taps; W.want(&d_taps, 2048);
    VP_TRY(vp_ws_commit(ctx, W, "vp_gaussian_blur_u8"));
    VP_TRY(h2d(ctx, d_src, src, nbytes));
    VP_TRY(h2d(ctx, d_taps, taps, (size_t)(kw + kh) * 2));
    VP_HIP(ctx, hipStreamSynchronize(ctx->stream));   // taps is a local array
    if (kw == 1 && kh == 1) { VP_TRY(d2h(ctx, dst, d_src, nbytes)); return vp_synchronize(ctx); }
    VP_TRY(vpk_gaussian_blur(ctx, d_src, w, h, cn, d_taps, kw, kh, d_tmp, d_dst));
    VP_TRY(d2h(ctx, dst, d_dst, nbytes));
    return vp_synchronize(ctx);
}

int vp_gaussian_blur_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, int cn, int kw, int kh, double sigma1, double sigma2,
                         uint8_t* d_dst)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(blur_args(ctx, "vp_gaussian_blur_dev arguments", d_src, d_dst, w, h, cn, kw, kh, &sigma1, &sigma2));
    const size_t rowbytes = (size_t)w * cn, nbytes = rowbytes * h;
    if (src_stride < rowbytes || dev_overlap(d_src, strided_bytes(src_stride, rowbytes, h), d_dst, nbytes))
        return vp_fail(ctx, VP_ERR_INVALID, "vp_gaussian_blur_dev: src_stride, or dst overlaps src");
    if (kw == 1 && kh == 1) {
        VP_HIP(ctx, hipMemcpy2DAsync(d_dst, rowbytes, d_src, src_stride, rowbytes, h, hipMemcpyDeviceToDevice, ctx->stream));
        return VP_OK;
    }
    const bool one = vp_gaussian_onepass_fits(kw, kh) && (ctx->opt.v[VP_OPT_BLUR_ONEPASS] == 1 || (ctx->opt.v[VP_OPT_BLUR_ONEPASS] < 0 && blur_onepass_measured_faster(cn, kw, kh)));
    vp_ws_frame W;
    uint16_t* d_taps; W.want(&d_taps, 2048);
    uint16_t* d_tmp = nullptr;
    if (!one) W.want(&d_tmp, nbytes * 2);
    VP_TRY(vp_ws_commit(ctx, W, "vp_gaussian_blur_dev"));
    // the taps go over in a pinned chunk of the context's ring: the copy is enqueued, nothing waits for it
    int slot = -1;
    uint16_t* taps = reinterpret_cast<uint16_t*>(vp_ring_take(ctx, 2048, &slot));
    if (!taps) return vp_fail(ctx, VP_ERR_NOMEM, "pinned staging");
    vp_gaussian_taps(kw, sigma1, taps);
    vp_gaussian_taps(kh, sigma2, taps + kw);
    int rc = h2d(ctx, d_taps, taps, (size_t)(kw + kh) * 2);
    if (rc == VP_OK) {
        if (one) rc = vpk_gaussian_blur_onepass(ctx, d_src, src_stride, w, h, cn, d_taps, kw, kh, d_dst);
        else rc = vpk_gaussian_blur(ctx, d_src, w, h, cn, d_taps, kw, kh, d_tmp, d_dst, src_stride);
    }
    vp_ring_done(ctx, slot);
    return rc;
}

// cv2.medianBlur: odd windows 1..255, 1..4 channels at every size (cv2's own limits on channels are the caller's business)
static int median_args(vp_ctx* ctx, const char* who, const void* src, const void* dst, int w, int h, int cn, int ksize)
{
    if (!src || !dst || w <= 0 || h <= 0 || h > 65535 || cn < 1 || cn > 4 || (size_t)w * cn > ((size_t)1 << 30) || ksize <= 0 || !(ksize & 1) || ksize > 255)
        return vp_fail(ctx, VP_ERR_INVALID, who);
    return VP_OK;
}

int vp_median_blur_u8(vp_ctx* ctx, const uint8_t* src, int w, int h, int cn, int ksize, uint8_t* dst)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(median_args(ctx, "vp_median_blur_u8 arguments", src, dst, w, h, cn, ksize));
    const size_t rowbytes = (size_t)w * cn, nbytes = rowbytes * h;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, nbytes);
    uint8_t* d_dst; W.want(&d_dst, nbytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_median_blur_u8"));
    VP_TRY(h2d(ctx, d_src, src, nbytes));
    VP_TRY(vpk_median_blur(ctx, d_src, rowbytes, w, h, cn, ksize, 0, nullptr, d_dst, nullptr, nullptr));
    VP_TRY(d2h(ctx, dst, d_dst, nbytes));
    return vp_synchronize(ctx);
}

int vp_median_blur_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, int cn, int ksize, int binary_hint,
                       const unsigned long long* d_src_bits, uint8_t* d_dst, unsigned long long* d_dst_bits, int* made_bits)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(median_args(ctx, "vp_median_blur_dev arguments", d_src, d_dst, w, h, cn, ksize));
    const size_t rowbytes = (size_t)w * cn, nbytes = rowbytes * h, sbytes = strided_bytes(src_stride, rowbytes, h);
    if (src_stride < rowbytes || dev_overlap(d_src, sbytes, d_dst, nbytes))
        return vp_fail(ctx, VP_ERR_INVALID, "vp_median_blur_dev: src_stride, or dst overlaps src");
    const size_t pbytes = (size_t)vp_ww(w) * 8 * h;
    if (((uintptr_t)d_src_bits | (uintptr_t)d_dst_bits) & 7u) return vp_fail(ctx, VP_ERR_INVALID, "vp_median_blur_dev: a bit plane is not 8-byte aligned");
    if ((d_src_bits && dev_overlap(d_src_bits, pbytes, d_dst, nbytes)) ||
        (d_dst_bits && (dev_overlap(d_dst_bits, pbytes, d_dst, nbytes) || dev_overlap(d_dst_bits, pbytes, d_src, sbytes) ||
                        (d_src_bits && dev_overlap(d_dst_bits, pbytes, d_src_bits, pbytes)))))
        return vp_fail(ctx, VP_ERR_INVALID, "vp_median_blur_dev: a bit plane overlaps an image it is not the plane of");
    return vpk_median_blur(ctx, d_src, src_stride, w, h, cn, ksize, binary_hint != 0, reinterpret_cast<const u64*>(d_src_bits), d_dst,
                           reinterpret_cast<u64*>(d_dst_bits), made_bits);
}

// cv2.Sobel / Scharr / Laplacian / spatialGradient: the plan is the argument check (vp_deriv_plan.h), shared by the four entries
static int deriv_args(vp_ctx* ctx, const char* who, const void* src, const void* dst, const void* dst2, int w, int h, int cn, int op, int dx, int dy, int ksize,
                      int ddepth, int border, vp_deriv_plan* P)
{
    if (!src || !dst || !dst2 || (op != VP_DERIV_SOBEL && op != VP_DERIV_SCHARR && op != VP_DERIV_LAPLACIAN && op != VP_DV_OP_SPATIAL_GRADIENT))
        return vp_fail(ctx, VP_ERR_INVALID, who);
    *P = vp_deriv_make_plan(w, h, cn, op, dx, dy, ksize, ddepth, border);
    if (!P->ok) return vp_fail(ctx, VP_ERR_INVALID, who);
    return VP_OK;
}

// what the device forms add: the stride, the destination's alignment to its element, and no overlap
static int deriv_dev_args(vp_ctx* ctx, const char* who, const void* d_src, size_t src_stride, size_t rowbytes, int h, const void* d_dst, size_t esize)
{
    if (src_stride < rowbytes || ((uintptr_t)d_dst & (esize - 1)) || dev_overlap(d_src, strided_bytes(src_stride, rowbytes, h), d_dst, rowbytes * h * esize))
        return vp_fail(ctx, VP_ERR_INVALID, who);
    return VP_OK;
}

int vp_deriv_u8(vp_ctx* ctx, const uint8_t* src, int w, int h, int cn, int op, int dx, int dy, int ksize, int ddepth, int border, void* dst)
{
    VP_TRY(check_ctx(ctx));
    vp_deriv_plan P;
    VP_TRY(deriv_args(ctx, "vp_deriv_u8 arguments", src, dst, dst, w, h, cn, op == VP_DV_OP_SPATIAL_GRADIENT ? -1 : op, dx, dy, ksize, ddepth, border, &P));
    const size_t rowbytes = (size_t)w * cn, nbytes = rowbytes * h, obytes = nbytes * P.esize;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, nbytes);
    uint8_t* d_dst; W.want(&d_dst, obytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_deriv_u8"));
    VP_TRY(h2d(ctx, d_src, src, nbytes));
    VP_TRY(vpk_deriv(ctx, d_src, rowbytes, w, h, cn, P, d_dst, nullptr));
    VP_TRY(d2h(ctx, dst, d_dst, obytes));
    return vp_synchronize(ctx);
}

int vp_deriv_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, int cn, int op, int dx, int dy, int ksize, int ddepth, int border, void* d_dst)
{
    VP_TRY(check_ctx(ctx));
    vp_deriv_plan P;
    VP_TRY(deriv_args(ctx, "vp_deriv_dev arguments", d_src, d_dst, d_dst, w, h, cn, op == VP_DV_OP_SPATIAL_GRADIENT ? -1 : op, dx, dy, ksize, ddepth, border, &P));
    VP_TRY(deriv_dev_args(ctx, "vp_deriv_dev: src_stride, dst is not aligned to its element, or dst overlaps src", d_src, src_stride, (size_t)w * cn, h, d_dst, P.esize));
    return vpk_deriv(ctx, d_src, src_stride, w, h, cn, P, d_dst, nullptr);
}

int vp_spatial_gradient_u8(vp_ctx* ctx, const uint8_t* src, int w, int h, int ksize, int border, int16_t* dx, int16_t* dy)
{
    VP_TRY(check_ctx(ctx));
    vp_deriv_plan P;
    VP_TRY(deriv_args(ctx, "vp_spatial_gradient_u8 arguments", src, dx, dy, w, h, 1, VP_DV_OP_SPATIAL_GRADIENT, 1, 1, ksize, VP_DEPTH_16S, border, &P));
    const size_t nbytes = (size_t)w * h, obytes = nbytes * 2;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, nbytes);
    uint8_t* d_dx; W.want(&d_dx, obytes);
    uint8_t* d_dy; W.want(&d_dy, obytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_spatial_gradient_u8"));
    VP_TRY(h2d(ctx, d_src, src, nbytes));
    VP_TRY(vpk_deriv(ctx, d_src, (size_t)w, w, h, 1, P, d_dx, d_dy));
    VP_TRY(d2h(ctx, dx, d_dx, obytes));
    VP_TRY(d2h(ctx, dy, d_dy, obytes));
    return vp_synchronize(ctx);
}

int vp_spatial_gradient_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, int ksize, int border, int16_t* d_dx, int16_t* d_dy)
{
    VP_TRY(check_ctx(ctx));
    vp_deriv_plan P;
    VP_TRY(deriv_args(ctx, "vp_spatial_gradient_dev arguments", d_src, d_dx, d_dy, w, h, 1, VP_DV_OP_SPATIAL_GRADIENT, 1, 1, ksize, VP_DEPTH_16S, border, &P));
    const char* who = "vp_spatial_gradient_dev: src_stride, a plane is not aligned to its element, or the planes overlap src or each other";
    VP_TRY(deriv_dev_args(ctx, who, d_src, src_stride, (size_t)w, h, d_dx, 2));
    VP_TRY(deriv_dev_args(ctx, who, d_src, src_stride, (size_t)w, h, d_dy, 2));
    if (dev_overlap(d_dx, (size_t)w * h * 2, d_dy, (size_t)w * h * 2)) return vp_fail(ctx, VP_ERR_INVALID, who);
    return vpk_deriv(ctx, d_src, src_stride, w, h, 1, P, d_dx, d_dy);
}

static int csa_args(vp_ctx* ctx, const char* who, const void* src, const void* dst, int depth, size_t n, size_t* esize)
{
    if (!src || !dst || n == 0 || n > ((size_t)1 << 36) || (depth != VP_DEPTH_8U && depth != VP_DEPTH_16S && depth != VP_DEPTH_32F && depth != VP_DEPTH_64F))
        return vp_fail(ctx, VP_ERR_INVALID, who);
    *esize = depth == VP_DEPTH_8U ? 1 : depth == VP_DEPTH_16S ? 2 : depth == VP_DEPTH_32F ? 4 : 8;
    return VP_OK;
}

int vp_convert_scale_abs_u8(vp_ctx* ctx, const void* src, int depth, size_t n, uint8_t* dst)
{
    VP_TRY(check_ctx(ctx));
    size_t esize;
    VP_TRY(csa_args(ctx, "vp_convert_scale_abs_u8 arguments", src, dst, depth, n, &esize));
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, n * esize);
    uint8_t* d_dst; W.want(&d_dst, n);
    VP_TRY(vp_ws_commit(ctx, W, "vp_convert_scale_abs_u8"));
    VP_TRY(h2d(ctx, d_src, src, n * esize));
    VP_TRY(vpk_convert_scale_abs(ctx, d_src, depth, n, d_dst));
    VP_TRY(d2h(ctx, dst, d_dst, n));
    return vp_synchronize(ctx);
}

int vp_convert_scale_abs_dev(vp_ctx* ctx, const void* d_src, int depth, size_t n, uint8_t* d_dst)
{
    VP_TRY(check_ctx(ctx));
    size_t esize;
    VP_TRY(csa_args(ctx, "vp_convert_scale_abs_dev arguments", d_src, d_dst, depth, n, &esize));
    if (((uintptr_t)d_src & (esize - 1)) || dev_overlap(d_src, n * esize, d_dst, n))
        return vp_fail(ctx, VP_ERR_INVALID, "vp_convert_scale_abs_dev: src is not aligned to its element, or dst overlaps src");
    return vpk_convert_scale_abs(ctx, d_src, depth, n, d_dst);
}

// cv2.boxFilter / blur, pyrDown, pyrUp, integral (vp_box_plan.h holds the checks).  An area's admission is enumerated once and kept.
int vp_box_area_exact(int area)
{
    static std::mutex mu;
    static std::vector<signed char> known;                   // 0: not asked yet, 1: refused, 2: admitted
    if (area < 1 || area > BX_MAXK * BX_MAXK) return -1;
    {
        std::lock_guard<std::mutex> g(mu);
        if (known.empty()) known.assign((size_t)BX_MAXK * BX_MAXK + 1, 0);
        if (known[area]) return known[area] - 1;
    }
    const int r = vp_box_area_admit(area);
    std::lock_guard<std::mutex> g(mu);
    known[area] = (signed char)(r + 1);
    return r;
}

static int box_args(vp_ctx* ctx, const char* who, const void* src, const void* dst, int w, int h, int cn, int kw, int kh, int normalize, int ddepth, int border,
                    vp_box_plan* P)
{
    if (!src || !dst) return vp_fail(ctx, VP_ERR_INVALID, who);
    *P = vp_box_make_plan(w, h, cn, kw, kh, normalize != 0, ddepth, border);
    if (!P->ok) return vp_fail(ctx, VP_ERR_INVALID, who);
    if (normalize) {
        if (vp_box_area_exact(kw * kh) != 1)
            return vp_fail(ctx, VP_ERR_INVALID, "box filter: OpenCV's roundings of sum / area disagree for this window area, it cannot be restated");
        P->div = vp_box_make_div(kw * kh);
    }
    return VP_OK;
}

// what the device forms of this family add: the stride, the destination's alignment to its element, and no overlap
static int box_dev_args(vp_ctx* ctx, const char* who, const void* d_src, size_t src_stride, size_t rowbytes, int h, const void* d_dst, size_t dbytes, size_t esize)
{
    if (src_stride < rowbytes || ((uintptr_t)d_dst & (esize - 1)) || dev_overlap(d_src, strided_bytes(src_stride, rowbytes, h), d_dst, dbytes))
        return vp_fail(ctx, VP_ERR_INVALID, who);
    return VP_OK;
}

int vp_box_filter_u8(vp_ctx* ctx, const uint8_t* src, int w, int h, int cn, int kw, int kh, int normalize, int ddepth, int border, void* dst)
{
    VP_TRY(check_ctx(ctx));
    vp_box_plan P;
    VP_TRY(box_args(ctx, "vp_box_filter_u8 arguments", src, dst, w, h, cn, kw, kh, normalize, ddepth, border, &P));
    const size_t rowbytes = (size_t)w * cn, nbytes = rowbytes * h, obytes = nbytes * P.esize, mbytes = vp_box_mid_bytes(w, h, cn, P);
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, nbytes);
    uint8_t* d_dst; W.want(&d_dst, obytes);
    uint16_t* d_mid = nullptr;
    if (mbytes) W.want(&d_mid, mbytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_box_filter_u8"));
    VP_TRY(h2d(ctx, d_src, src, nbytes));
    VP_TRY(vpk_box_filter(ctx, d_src, rowbytes, w, h, cn, P, d_mid, d_dst));
    VP_TRY(d2h(ctx, dst, d_dst, obytes));
    return vp_synchronize(ctx);
}

int vp_box_filter_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, int cn, int kw, int kh, int normalize, int ddepth, int border, void* d_dst)
{
    VP_TRY(check_ctx(ctx));
    vp_box_plan P;
    VP_TRY(box_args(ctx, "vp_box_filter_dev arguments", d_src, d_dst, w, h, cn, kw, kh, normalize, ddepth, border, &P));
    const size_t rowbytes = (size_t)w * cn, mbytes = vp_box_mid_bytes(w, h, cn, P);
    VP_TRY(box_dev_args(ctx, "vp_box_filter_dev: src_stride, dst is not aligned to its element, or dst overlaps src", d_src, src_stride, rowbytes, h, d_dst,
                        rowbytes * h * P.esize, P.esize));
    uint16_t* d_mid = nullptr;
    if (mbytes) {
        vp_ws_frame W;
        W.want(&d_mid, mbytes);
        VP_TRY(vp_ws_commit(ctx, W, "vp_box_filter_dev"));
    }
    return vpk_box_filter(ctx, d_src, src_stride, w, h, cn, P, d_mid, d_dst);
}

static int pyr_args(vp_ctx* ctx, const char* who, const void* src, const void* dst, int w, int h, int cn, int border, bool down)
{
    if (!src || !dst || !vp_pyr_sizes_ok(w, h, cn) || (down && !vp_pyr_down_border_ok(border))) return vp_fail(ctx, VP_ERR_INVALID, who);
    return VP_OK;
}

int vp_pyr_down_u8(vp_ctx* ctx, const uint8_t* src, int w, int h, int cn, int border, uint8_t* dst)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(pyr_args(ctx, "vp_pyr_down_u8 arguments", src, dst, w, h, cn, border, true));
    const size_t nbytes = (size_t)w * cn * h, obytes = (size_t)((w + 1) / 2) * cn * ((h + 1) / 2);
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, nbytes);
    uint8_t* d_dst; W.want(&d_dst, obytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_pyr_down_u8"));
    VP_TRY(h2d(ctx, d_src, src, nbytes));
    VP_TRY(vpk_pyr_down(ctx, d_src, (size_t)w * cn, w, h, cn, border & ~VP_BORDER_ISOLATED, d_dst));
    VP_TRY(d2h(ctx, dst, d_dst, obytes));
    return vp_synchronize(ctx);
}

int vp_pyr_down_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, int cn, int border, uint8_t* d_dst)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(pyr_args(ctx, "vp_pyr_down_dev arguments", d_src, d_dst, w, h, cn, border, true));
    VP_TRY(box_dev_args(ctx, "vp_pyr_down_dev: src_stride, or dst overlaps src", d_src, src_stride, (size_t)w * cn, h, d_dst,
                        (size_t)((w + 1) / 2) * cn * ((h + 1) / 2), 1));
    return vpk_pyr_down(ctx, d_src, src_stride, w, h, cn, border & ~VP_BORDER_ISOLATED, d_dst);
}

int vp_pyr_up_u8(vp_ctx* ctx, const uint8_t* src, int w, int h, int cn, uint8_t* dst)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(pyr_args(ctx, "vp_pyr_up_u8 arguments", src, dst, w, h, cn, 0, false));
    const size_t nbytes = (size_t)w * cn * h, obytes = 4 * nbytes;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, nbytes);
    uint8_t* d_dst; W.want(&d_dst, obytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_pyr_up_u8"));
    VP_TRY(h2d(ctx, d_src, src, nbytes));
    VP_TRY(vpk_pyr_up(ctx, d_src, (size_t)w * cn, w, h, cn, d_dst));
    VP_TRY(d2h(ctx, dst, d_dst, obytes));
    return vp_synchronize(ctx);
}

int vp_pyr_up_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, int cn, uint8_t* d_dst)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(pyr_args(ctx, "vp_pyr_up_dev arguments", d_src, d_dst, w, h, cn, 0, false));
    VP_TRY(box_dev_args(ctx, "vp_pyr_up_dev: src_stride, or dst overlaps src", d_src, src_stride, (size_t)w * cn, h, d_dst, (size_t)4 * w * cn * h, 1));
    return vpk_pyr_up(ctx, d_src, src_stride, w, h, cn, d_dst);
}

static int integral_args(vp_ctx* ctx, const char* who, const void* src, const void* dst, int w, int h, int cn)
{
    if (!src || !dst || cn < 1 || cn > 4 || w <= 0 || h <= 0) return vp_fail(ctx, VP_ERR_INVALID, who);
    if (!vp_integral_sizes_ok(w, h, cn)) return vp_fail(ctx, VP_ERR_INVALID, "integral: 255 * w * h does not fit the int32 sums");
    return VP_OK;
}

int vp_integral_u8(vp_ctx* ctx, const uint8_t* src, int w, int h, int cn, int32_t* dst)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(integral_args(ctx, "vp_integral_u8 arguments", src, dst, w, h, cn));
    const size_t nbytes = (size_t)w * cn * h, obytes = (size_t)(w + 1) * cn * (h + 1) * 4;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, nbytes);
    int32_t* d_dst; W.want(&d_dst, obytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_integral_u8"));
    VP_TRY(h2d(ctx, d_src, src, nbytes));
    VP_TRY(vpk_integral(ctx, d_src, (size_t)w * cn, w, h, cn, d_dst));
    VP_TRY(d2h(ctx, dst, d_dst, obytes));
    return vp_synchronize(ctx);
}

int vp_integral_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, int cn, int32_t* d_dst)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(integral_args(ctx, "vp_integral_dev arguments", d_src, d_dst, w, h, cn));
    VP_TRY(box_dev_args(ctx, "vp_integral_dev: src_stride, dst is not aligned to int32, or dst overlaps src", d_src, src_stride, (size_t)w * cn, h, d_dst,
                        (size_t)(w + 1) * cn * (h + 1) * 4, 4));
    return vpk_integral(ctx, d_src, src_stride, w, h, cn, d_dst);
}

static int resize_args(vp_ctx* ctx, const char* who, const void* src, const void* dst, int w, int h, int cn, int dw, int dh, double inv_sx, double inv_sy)
{
    if (!src || !dst || w <= 0 || h <= 0 || dw <= 0 || dh <= 0 || dh > 65535 || cn < 1 || cn > 4 || !std::isfinite(inv_sx) || !std::isfinite(inv_sy) ||
        !(inv_sx > 0) || !(inv_sy > 0))
        return vp_fail(ctx, VP_ERR_INVALID, who);
    return VP_OK;
}

int vp_resize_u8_scaled(vp_ctx* ctx, const uint8_t* src, int w, int h, int cn, int dw, int dh, double inv_sx, double inv_sy, uint8_t* dst)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(resize_args(ctx, "vp_resize_u8 arguments", src, dst, w, h, cn, dw, dh, inv_sx, inv_sy));
    const size_t sbytes = (size_t)w * h * cn, dbytes = (size_t)dw * dh * cn;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, sbytes);
    uint8_t* d_dst; W.want(&d_dst, dbytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_resize_u8_scaled"));
    VP_TRY(h2d(ctx, d_src, src, sbytes));
    VP_TRY(vpk_resize_u8(ctx, d_src, w, h, cn, dw, dh, inv_sx, inv_sy, d_dst));
    VP_TRY(d2h(ctx, dst, d_dst, dbytes));
    return vp_synchronize(ctx);
}

int vp_resize_u8(vp_ctx* ctx, const uint8_t* src, int w, int h, int cn, int dw, int dh, uint8_t* dst)
{
    // cv::resize with a dsize: inv_scale = (double)dsize / ssize (an empty source is rejected by the scaled entry)
    return vp_resize_u8_scaled(ctx, src, w, h, cn, dw, dh, w > 0 ? (double)dw / w : 0.0, h > 0 ? (double)dh / h : 0.0, dst);
}

int vp_resize_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, int cn, int dw, int dh, double inv_sx, double inv_sy, uint8_t* d_dst)
{
    VP_TRY(check_ctx(ctx));
    if (inv_sx <= 0 && inv_sy <= 0) {                    // cv::resize with a dsize: inv_scale = (double)dsize / ssize
        inv_sx = w > 0 ? (double)dw / w : 0.0;
        inv_sy = h > 0 ? (double)dh / h : 0.0;
    }
    VP_TRY(resize_args(ctx, "vp_resize_dev arguments", d_src, d_dst, w, h, cn, dw, dh, inv_sx, inv_sy));
    const size_t rowbytes = (size_t)w * cn;
    if (src_stride < rowbytes || dev_overlap(d_src, strided_bytes(src_stride, rowbytes, h), d_dst, (size_t)dw * dh * cn))
        return vp_fail(ctx, VP_ERR_INVALID, "vp_resize_dev: src_stride, or dst overlaps src");
    return vpk_resize_u8(ctx, d_src, w, h, cn, dw, dh, inv_sx, inv_sy, d_dst, src_stride);
}

static int warp_args(vp_ctx* ctx, const char* who, const void* src, const void* dst, int w, int h, int cn, const double* m23, int flags, int border_mode,
                     int dw, int dh)
{
    if (!src || !dst || !m23 || w <= 0 || h <= 0 || dw <= 0 || dh <= 0 || dh > 65535 || cn < 1 || cn > 4 || (flags & ~VP_WARP_INVERSE_MAP) ||
        (border_mode != VP_BORDER_CONSTANT && border_mode != VP_BORDER_REPLICATE))
        return vp_fail(ctx, VP_ERR_INVALID, who);
    for (int i = 0; i < 6; i++)
        if (!std::isfinite(m23[i])) return vp_fail(ctx, VP_ERR_INVALID, "warp affine: matrix is not finite");
    return VP_OK;
}

int vp_warp_affine_u8(vp_ctx* ctx, const uint8_t* src, int w, int h, int cn, const double* m23, int flags, int border_mode,
                      const uint8_t* border_value, uint8_t* dst, int dw, int dh)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(warp_args(ctx, "vp_warp_affine_u8 arguments", src, dst, w, h, cn, m23, flags, border_mode, dw, dh));
    const size_t sbytes = (size_t)w * h * cn, dbytes = (size_t)dw * dh * cn;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, sbytes);
    uint8_t* d_dst; W.want(&d_dst, dbytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_warp_affine_u8"));
    VP_TRY(h2d(ctx, d_src, src, sbytes));
    VP_TRY(vpk_warp_affine_u8(ctx, d_src, w, h, cn, m23, (flags & VP_WARP_INVERSE_MAP) != 0, border_mode, border_value, d_dst, dw, dh));
    VP_TRY(d2h(ctx, dst, d_dst, dbytes));
    return vp_synchronize(ctx);
}

int vp_warp_affine_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, int cn, const double* m23, int flags, int border_mode,
                       const uint8_t* border_value, uint8_t* d_dst, int dw, int dh)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(warp_args(ctx, "vp_warp_affine_dev arguments", d_src, d_dst, w, h, cn, m23, flags, border_mode, dw, dh));
    const size_t rowbytes = (size_t)w * cn;
    if (src_stride < rowbytes || dev_overlap(d_src, strided_bytes(src_stride, rowbytes, h), d_dst, (size_t)dw * dh * cn))
        return vp_fail(ctx, VP_ERR_INVALID, "vp_warp_affine_dev: src_stride, or dst overlaps src");
    // the matrix and the border value travel as kernel arguments
    return vpk_warp_affine_u8(ctx, d_src, w, h, cn, m23, (flags & VP_WARP_INVERSE_MAP) != 0, border_mode, border_value, d_dst, dw, dh, src_stride);
}

// cv2.remap / convertMaps / warpPerspective (vp_remap.hip).  One check per family; `maps`: the map planes and their bytes, all of
// which the destination must stay clear of (device forms).
static int gather_args(vp_ctx* ctx, const char* who, const void* src, const void* dst, int w, int h, int cn, int dw, int dh, int interp, int border_mode)
{
    if (!src || !dst || !vp_remap_sizes_ok(w, h, cn, dw, dh) || (interp != VP_INTER_NEAREST && interp != VP_INTER_LINEAR) ||
        (border_mode != VP_BORDER_CONSTANT && border_mode != VP_BORDER_REPLICATE))
        return vp_fail(ctx, VP_ERR_INVALID, who);
    return VP_OK;
}
static int gather_dev_args(vp_ctx* ctx, const char* who, const uint8_t* d_src, size_t src_stride, int w, int h, int cn, const uint8_t* d_dst, int dw, int dh,
                           const void* map0, size_t bytes0, const void* map1, size_t bytes1)
{
    const size_t rowbytes = (size_t)w * cn, dbytes = (size_t)dw * dh * cn;
    if (src_stride < rowbytes || dev_overlap(d_src, strided_bytes(src_stride, rowbytes, h), d_dst, dbytes) || (map0 && dev_overlap(map0, bytes0, d_dst, dbytes)) ||
        (map1 && dev_overlap(map1, bytes1, d_dst, dbytes)))
        return vp_fail(ctx, VP_ERR_INVALID, who);
    return VP_OK;
}

int vp_convert_maps_dev(vp_ctx* ctx, const float* mapx, const float* mapy, int mw, int mh, int nearest, int16_t* xy_out, uint16_t* frac_out)
{
    VP_TRY(check_ctx(ctx));
    if (!mapx || !xy_out || !vp_remap_map_ok(mw, mh) || (nearest ? frac_out != nullptr : frac_out == nullptr))
        return vp_fail(ctx, VP_ERR_INVALID, "vp_convert_maps_dev arguments");
    const size_t n = (size_t)mw * mh, inx = n * (mapy ? 4 : 8);
    const void* outs[2] = {xy_out, frac_out};
    const size_t outb[2] = {n * 4, n * 2};
    for (int o = 0; o < 2; o++)
        if (outs[o] && (dev_overlap(mapx, inx, outs[o], outb[o]) || (mapy && dev_overlap(mapy, n * 4, outs[o], outb[o]))))
            return vp_fail(ctx, VP_ERR_INVALID, "vp_convert_maps_dev: an output overlaps a map");
    if (frac_out && dev_overlap(xy_out, n * 4, frac_out, n * 2)) return vp_fail(ctx, VP_ERR_INVALID, "vp_convert_maps_dev: the outputs overlap");
    return vpk_convert_maps(ctx, mapx, mapy, mw, mh, nearest != 0, xy_out, frac_out);
}

int vp_remap_fixed_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, int cn, const int16_t* xy, const uint16_t* frac, int mw, int mh,
                       int interp, int border_mode, const uint8_t* border_value, uint8_t* d_dst)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(gather_args(ctx, "vp_remap_fixed_dev arguments", d_src, d_dst, w, h, cn, mw, mh, interp, border_mode));
    if (!xy || (interp == VP_INTER_NEAREST ? frac != nullptr : frac == nullptr))
        return vp_fail(ctx, VP_ERR_INVALID, "vp_remap_fixed_dev: nearest takes the x,y plane alone, linear needs the fraction plane");
    const size_t n = (size_t)mw * mh;
    VP_TRY(gather_dev_args(ctx, "vp_remap_fixed_dev: src_stride, or dst overlaps src or a map", d_src, src_stride, w, h, cn, d_dst, mw, mh, xy, n * 4, frac, n * 2));
    return vpk_remap_fixed(ctx, d_src, src_stride, w, h, cn, xy, frac, mw, mh, interp == VP_INTER_LINEAR, border_mode, border_value, d_dst);
}

int vp_remap_f32_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, int cn, const float* mapx, const float* mapy, int mw, int mh, int interp,
                     int border_mode, const uint8_t* border_value, uint8_t* d_dst)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(gather_args(ctx, "vp_remap_f32_dev arguments", d_src, d_dst, w, h, cn, mw, mh, interp, border_mode));
    if (!mapx) return vp_fail(ctx, VP_ERR_INVALID, "vp_remap_f32_dev: no map");
    const size_t n = (size_t)mw * mh;
    VP_TRY(gather_dev_args(ctx, "vp_remap_f32_dev: src_stride, or dst overlaps src or a map", d_src, src_stride, w, h, cn, d_dst, mw, mh, mapx, n * (mapy ? 4 : 8),
                           mapy, n * 4));
    return vpk_remap_f32(ctx, d_src, src_stride, w, h, cn, mapx, mapy, mw, mh, interp == VP_INTER_LINEAR, border_mode, border_value, d_dst);
}

int vp_remap_u8(vp_ctx* ctx, const uint8_t* src, int w, int h, int cn, const float* mapx, const float* mapy, int mw, int mh, int interp, int border_mode,
                const uint8_t* border_value, uint8_t* dst)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(gather_args(ctx, "vp_remap_u8 arguments", src, dst, w, h, cn, mw, mh, interp, border_mode));
    if (!mapx) return vp_fail(ctx, VP_ERR_INVALID, "vp_remap_u8: no map");
    const size_t n = (size_t)mw * mh, sbytes = (size_t)w * h * cn, dbytes = n * cn, xbytes = n * (mapy ? 4 : 8), ybytes = mapy ? n * 4 : 0;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, sbytes);
    uint8_t* d_dst; W.want(&d_dst, dbytes);
    float* d_mx; W.want(&d_mx, xbytes);
    float* d_my = nullptr;
    if (mapy) W.want(&d_my, ybytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_remap_u8"));
    VP_TRY(h2d(ctx, d_src, src, sbytes));
    VP_TRY(h2d(ctx, d_mx, mapx, xbytes));
    if (mapy) VP_TRY(h2d(ctx, d_my, mapy, ybytes));
    VP_TRY(vpk_remap_f32(ctx, d_src, 0, w, h, cn, d_mx, d_my, mw, mh, interp == VP_INTER_LINEAR, border_mode, border_value, d_dst));
    VP_TRY(d2h(ctx, dst, d_dst, dbytes));
    return vp_synchronize(ctx);
}

static int wp_args(vp_ctx* ctx, const char* who, const void* src, const void* dst, int w, int h, int cn, const double* m33, int flags, int border_mode, int dw, int dh)
{
    if (!m33 || (flags & ~(VP_WARP_INVERSE_MAP | VP_INTER_LINEAR))) return vp_fail(ctx, VP_ERR_INVALID, who);
    VP_TRY(gather_args(ctx, who, src, dst, w, h, cn, dw, dh, flags & ~VP_WARP_INVERSE_MAP, border_mode));
    for (int i = 0; i < 9; i++)
        if (!std::isfinite(m33[i])) return vp_fail(ctx, VP_ERR_INVALID, "warp perspective: matrix is not finite");
    return VP_OK;
}

int vp_warp_perspective_u8(vp_ctx* ctx, const uint8_t* src, int w, int h, int cn, const double* m33, int flags, int border_mode, const uint8_t* border_value,
                           uint8_t* dst, int dw, int dh)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(wp_args(ctx, "vp_warp_perspective_u8 arguments", src, dst, w, h, cn, m33, flags, border_mode, dw, dh));
    const size_t sbytes = (size_t)w * h * cn, dbytes = (size_t)dw * dh * cn;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, sbytes);
    uint8_t* d_dst; W.want(&d_dst, dbytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_warp_perspective_u8"));
    VP_TRY(h2d(ctx, d_src, src, sbytes));
    VP_TRY(vpk_warp_perspective(ctx, d_src, 0, w, h, cn, m33, (flags & VP_WARP_INVERSE_MAP) != 0, (flags & VP_INTER_LINEAR) != 0, border_mode, border_value, d_dst,
                                dw, dh));
    VP_TRY(d2h(ctx, dst, d_dst, dbytes));
    return vp_synchronize(ctx);
}

int vp_warp_perspective_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, int cn, const double* m33, int flags, int border_mode,
                            const uint8_t* border_value, uint8_t* d_dst, int dw, int dh)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(wp_args(ctx, "vp_warp_perspective_dev arguments", d_src, d_dst, w, h, cn, m33, flags, border_mode, dw, dh));
    VP_TRY(gather_dev_args(ctx, "vp_warp_perspective_dev: src_stride, or dst overlaps src", d_src, src_stride, w, h, cn, d_dst, dw, dh, nullptr, 0, nullptr, 0));
    return vpk_warp_perspective(ctx, d_src, src_stride, w, h, cn, m33, (flags & VP_WARP_INVERSE_MAP) != 0, (flags & VP_INTER_LINEAR) != 0, border_mode, border_value,
                                d_dst, dw, dh);
}

// cv2.adaptiveThreshold, mean (blocks up to 151) and Gaussian (up to VP_AGAUSS_MAX_BLOCK): maxValue rounded into [0, 255], C rounded
// away from the comparison (cv2's ceil for BINARY, floor for BINARY_INV)
static int adaptive_args(vp_ctx* ctx, const char* who, const void* src, const void* dst, int w, int h, double max_value, int type, int block, int max_block,
                         double c, int* imax, int* idelta)
{
    if (!src || !dst || w <= 0 || h <= 0 || h > 65535 || (type != VP_THRESH_BINARY && type != VP_THRESH_BINARY_INV) || !std::isfinite(max_value) ||
        !std::isfinite(c) || std::fabs(c) > 1e6)
        return vp_fail(ctx, VP_ERR_INVALID, who);
    if (block < 3 || (block & 1) == 0) return vp_fail(ctx, VP_ERR_INVALID, "adaptive threshold: block size must be odd and > 1");
    if (block > max_block) return vp_fail(ctx, VP_ERR_UNSUPPORTED, "adaptive threshold: block size above 151 (mean) / 511 (Gaussian)");
    *imax = (int)std::min(255.0, std::max(0.0, std::nearbyint(max_value)));
    *idelta = type == VP_THRESH_BINARY ? (int)std::ceil(c) : (int)std::floor(c);
    return VP_OK;
}

int vp_adaptive_threshold_mean_u8(vp_ctx* ctx, const uint8_t* src, int w, int h, double max_value, int type, int block, double c, uint8_t* dst)
{
    VP_TRY(check_ctx(ctx));
    int imax, idelta;
    VP_TRY(adaptive_args(ctx, "vp_adaptive_threshold_mean_u8 arguments", src, dst, w, h, max_value, type, block, 151, c, &imax, &idelta));
    const size_t npx = (size_t)w * h;
    if (max_value < 0) { memset(dst, 0, npx); return VP_OK; }
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, npx);
    uint8_t* d_dst; W.want(&d_dst, npx);
    uint16_t* d_tmp; W.want(&d_tmp, npx * 2);
    VP_TRY(vp_ws_commit(ctx, W, "vp_adaptive_threshold_mean_u8"));
    VP_TRY(h2d(ctx, d_src, src, npx));
    VP_TRY(vpk_adaptive_threshold_mean(ctx, d_src, w, h, imax, idelta, type == VP_THRESH_BINARY_INV, block, d_tmp, d_dst));
    VP_TRY(d2h(ctx, dst, d_dst, npx));
    return vp_synchronize(ctx);
}

int vp_adaptive_threshold_mean_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, double max_value, int type, int block, double c,
                                   uint8_t* d_dst)
{
    VP_TRY(check_ctx(ctx));
    int imax, idelta;
    VP_TRY(adaptive_args(ctx, "vp_adaptive_threshold_mean_dev arguments", d_src, d_dst, w, h, max_value, type, block, 151, c, &imax, &idelta));
    const size_t npx = (size_t)w * h;
    if (src_stride < (size_t)w || dev_overlap(d_src, strided_bytes(src_stride, (size_t)w, h), d_dst, npx))
        return vp_fail(ctx, VP_ERR_INVALID, "vp_adaptive_threshold_mean_dev: src_stride, or dst overlaps src");
    if (max_value < 0) {
        VP_HIP(ctx, hipMemsetAsync(d_dst, 0, npx, ctx->stream));
        return VP_OK;
    }
    vp_ws_frame W;
    uint16_t* d_tmp; W.want(&d_tmp, npx * 2);
    VP_TRY(vp_ws_commit(ctx, W, "vp_adaptive_threshold_mean_dev"));
    return vpk_adaptive_threshold_mean(ctx, d_src, w, h, imax, idelta, type == VP_THRESH_BINARY_INV, block, d_tmp, d_dst, src_stride);
}

// n frames in HBM -> packed (n, h, w) dst in HBM, enqueued on the context's stream; max_value < 0 gives zeros, as cv2 does
static int agauss_run(vp_ctx* ctx, const uint8_t* d_src, size_t stride, size_t fstride, int n, int w, int h, double max_value, int imax, int idelta, int inv,
                      int block, uint64_t* d_tmp, uint8_t* d_dst)
{
    if (max_value < 0) {
        VP_HIP(ctx, hipMemsetAsync(d_dst, 0, (size_t)n * w * h, ctx->stream));
        return VP_OK;
    }
    return vpk_adaptive_threshold_gaussian(ctx, d_src, stride, fstride, n, w, h, imax, idelta, inv, block, d_tmp, d_dst);
}

int vp_adaptive_threshold_gaussian_u8(vp_ctx* ctx, const uint8_t* src, int w, int h, double max_value, int type, int block, double c, uint8_t* dst)
{
    VP_TRY(check_ctx(ctx));
    int imax, idelta;
    VP_TRY(adaptive_args(ctx, "vp_adaptive_threshold_gaussian arguments", src, dst, w, h, max_value, type, block, VP_AGAUSS_MAX_BLOCK, c, &imax, &idelta));
    const size_t npx = (size_t)w * h;
    if (max_value < 0) { memset(dst, 0, npx); return VP_OK; }
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, npx);
    uint8_t* d_dst; W.want(&d_dst, npx);
    uint64_t* d_tmp; W.want(&d_tmp, vp_agauss_tmp_bytes(w, h, 1));
    VP_TRY(vp_ws_commit(ctx, W, "vp_adaptive_threshold_gaussian_u8"));
    VP_TRY(h2d(ctx, d_src, src, npx));
    VP_TRY(agauss_run(ctx, d_src, (size_t)w, npx, 1, w, h, max_value, imax, idelta, type == VP_THRESH_BINARY_INV, block, d_tmp, d_dst));
    VP_TRY(d2h(ctx, dst, d_dst, npx));
    return vp_synchronize(ctx);
}

int vp_adaptive_threshold_gaussian_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, double max_value, int type, int block,
                                       double c, uint8_t* d_dst)
{
    VP_TRY(check_ctx(ctx));
    int imax, idelta;
    VP_TRY(adaptive_args(ctx, "vp_adaptive_threshold_gaussian arguments", d_src, d_dst, w, h, max_value, type, block, VP_AGAUSS_MAX_BLOCK, c, &imax, &idelta));
    if (src_stride < (size_t)w) return vp_fail(ctx, VP_ERR_INVALID, "vp_adaptive_threshold_gaussian_dev src_stride");
    vp_ws_frame W;
    uint64_t* d_tmp; W.want(&d_tmp, vp_agauss_tmp_bytes(w, h, 1));
    VP_TRY(vp_ws_commit(ctx, W, "vp_adaptive_threshold_gaussian_dev"));
    return agauss_run(ctx, d_src, src_stride, src_stride * h, 1, w, h, max_value, imax, idelta, type == VP_THRESH_BINARY_INV, block, d_tmp, d_dst);
}

int vp_adaptive_threshold_gaussian_batch_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, size_t frame_stride, int n, int w, int h,
                                             double max_value, int type, int block, double c, uint8_t* d_dst)
{
    VP_TRY(check_ctx(ctx));
    int imax, idelta;
    VP_TRY(adaptive_args(ctx, "vp_adaptive_threshold_gaussian arguments", d_src, d_dst, w, h, max_value, type, block, VP_AGAUSS_MAX_BLOCK, c, &imax, &idelta));
    if (n <= 0 || n > 65535 || src_stride < (size_t)w || (n > 1 && frame_stride < src_stride * h))
        return vp_fail(ctx, VP_ERR_INVALID, "vp_adaptive_threshold_gaussian_batch_dev strides / frame count");
    vp_ws_frame W;
    uint64_t* d_tmp; W.want(&d_tmp, vp_agauss_tmp_bytes(w, h, n));
    VP_TRY(vp_ws_commit(ctx, W, "vp_adaptive_threshold_gaussian_batch_dev"));
    return agauss_run(ctx, d_src, src_stride, frame_stride, n, w, h, max_value, imax, idelta, type == VP_THRESH_BINARY_INV, block, d_tmp, d_dst);
}

// cv2.Canny thresholds: ordered, floored, held inside what the integer gradient magnitude can reach
static int canny_args(vp_ctx* ctx, const char* who, const void* src, const void* dst, int w, int h, int cn, double t1, double t2, int* low, int* high)
{
    if (!src || !dst || w <= 0 || h <= 0 || h > 65535 || (size_t)w * h > ((size_t)1 << 30) || cn < 1 || cn > 4 || !std::isfinite(t1) || !std::isfinite(t2))
        return vp_fail(ctx, VP_ERR_INVALID, who);
    if (t1 > t2) std::swap(t1, t2);
    *low = (int)std::floor(std::min(std::max(t1, -1.0), 1e9));
    *high = (int)std::floor(std::min(std::max(t2, -1.0), 1e9));
    return VP_OK;
}

int vp_canny_u8(vp_ctx* ctx, const uint8_t* src, int w, int h, int cn, double t1, double t2, uint8_t* dst)
{
    VP_TRY(check_ctx(ctx));
    int low, high;
    VP_TRY(canny_args(ctx, "vp_canny_u8 arguments", src, dst, w, h, cn, t1, t2, &low, &high));
    const size_t npx = (size_t)w * h;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, npx * cn);
    uint8_t* d_dst; W.want(&d_dst, npx);
    vp_canny_ws cw;
    vp_canny_want(W, w, h, &cw);
    VP_TRY(vp_ws_commit(ctx, W, "vp_canny_u8"));
    VP_TRY(h2d(ctx, d_src, src, npx * cn));
    VP_TRY(vpk_canny_u8(ctx, d_src, w, h, cn, low, high, d_dst, cw));
    VP_TRY(d2h(ctx, dst, d_dst, npx));
    return vp_synchronize(ctx);
}

// canny -> find_lines without leaving HBM: the same kernels as vp_canny_u8 on a device image; enqueued, not synchronised
int vp_canny_u8_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, int cn, double t1, double t2, uint8_t* d_dst)
{
    VP_TRY(check_ctx(ctx));
    int low, high;
    VP_TRY(canny_args(ctx, "vp_canny_u8_dev arguments", d_src, d_dst, w, h, cn, t1, t2, &low, &high));
    if (src_stride < (size_t)w * cn) return vp_fail(ctx, VP_ERR_INVALID, "vp_canny_u8_dev src_stride");
    const size_t npx = (size_t)w * h;
    const bool packed = src_stride == (size_t)w * cn;
    vp_ws_frame W;
    uint8_t* d_pk = nullptr;
    if (!packed) W.want(&d_pk, npx * cn);
    vp_canny_ws cw;
    vp_canny_want(W, w, h, &cw);
    VP_TRY(vp_ws_commit(ctx, W, "vp_canny_u8_dev"));
    const uint8_t* src = d_src;
    if (!packed) {
        VP_HIP(ctx, hipMemcpy2DAsync(d_pk, (size_t)w * cn, d_src, src_stride, (size_t)w * cn, h, hipMemcpyDeviceToDevice, ctx->stream));
        src = d_pk;
    }
    return vpk_canny_u8(ctx, src, w, h, cn, low, high, d_dst, cw);
}

static int hough_args(vp_ctx* ctx, const void* src, int w, int h, float* lines, int max_lines, int* n_lines)
{
    if (!src || !n_lines || w <= 0 || h <= 0 || w > 65535 || h > 65535 || max_lines < 0 || (max_lines > 0 && !lines))
        return vp_fail(ctx, VP_ERR_INVALID, "hough lines arguments");
    return VP_OK;
}

int vp_hough_lines_u8(vp_ctx* ctx, const uint8_t* src, int w, int h, double rho, double theta, int threshold, double min_theta, double max_theta,
                      float* lines, int max_lines, int* n_lines)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(hough_args(ctx, src, w, h, lines, max_lines, n_lines));
    return vp_hough_run(ctx, nullptr, src, w, (size_t)w * h, 1, w, h, rho, theta, threshold, min_theta, max_theta, lines, max_lines, n_lines);
}

int vp_hough_lines_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, double rho, double theta, int threshold,
                       double min_theta, double max_theta, float* lines, int max_lines, int* n_lines)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(hough_args(ctx, d_src, w, h, lines, max_lines, n_lines));
    if (src_stride < (size_t)w) return vp_fail(ctx, VP_ERR_INVALID, "src_stride");
    return vp_hough_run(ctx, d_src, nullptr, src_stride, src_stride * h, 1, w, h, rho, theta, threshold, min_theta, max_theta, lines, max_lines, n_lines);
}

int vp_hough_lines_batch_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, size_t frame_stride, int n, int w, int h, double rho,
                             double theta, int threshold, double min_theta, double max_theta, float* lines, int max_lines, int* n_lines)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(hough_args(ctx, d_src, w, h, lines, max_lines, n_lines));
    if (n <= 0 || n > 65535 || src_stride < (size_t)w || (n > 1 && frame_stride < src_stride * (h - 1) + w))
        return vp_fail(ctx, VP_ERR_INVALID, "vp_hough_lines_batch_dev strides / frame count");
    return vp_hough_run(ctx, d_src, nullptr, src_stride, frame_stride, n, w, h, rho, theta, threshold, min_theta, max_theta, lines, max_lines, n_lines);
}

int vp_hough_circles_u8(vp_ctx* ctx, const uint8_t* src, int w, int h, double dp, double min_dist, double param1, double param2, int min_radius,
                        int max_radius, float* circles, int max_circles, int* n_circles)
{
    VP_TRY(check_ctx(ctx));
    if (!src) return vp_fail(ctx, VP_ERR_INVALID, "hough circles arguments");
    return vp_hough_circles_run(ctx, nullptr, src, (size_t)w, w, h, dp, min_dist, param1, param2, min_radius, max_radius, circles, max_circles,
                                n_circles);
}

int vp_hough_circles_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, double dp, double min_dist, double param1,
                         double param2, int min_radius, int max_radius, float* circles, int max_circles, int* n_circles)
{
    VP_TRY(check_ctx(ctx));
    if (!d_src) return vp_fail(ctx, VP_ERR_INVALID, "hough circles arguments");
    return vp_hough_circles_run(ctx, d_src, nullptr, src_stride, w, h, dp, min_dist, param1, param2, min_radius, max_radius, circles,
                                max_circles, n_circles);
}

static int check_lb(vp_ctx* ctx, const void* src, const void* dst, int w, int h, int dw, int dh, int pad)
{
    if (!src || !dst || w <= 0 || h <= 0 || dw <= 0 || dh <= 0 || dh > 65535 || pad < 0 || pad > 255) return vp_fail(ctx, VP_ERR_INVALID, "letterbox arguments");
    return VP_OK;
}

int vp_letterbox_u8_f32(vp_ctx* ctx, const uint8_t* src, int w, int h, int dw, int dh, int pad, float* dst, float* geom_out)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(check_lb(ctx, src, dst, w, h, dw, dh, pad));
    const size_t sbytes = (size_t)w * h * 3, dbytes = (size_t)dw * dh * 12;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, sbytes);
    float* d_dst; W.want(&d_dst, dbytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_letterbox_u8_f32"));
    VP_TRY(h2d(ctx, d_src, src, sbytes));
    VP_TRY(vpk_letterbox(ctx, d_src, w, h, dw, dh, pad, d_dst, geom_out));
    VP_TRY(d2h(ctx, dst, d_dst, dbytes));
    return vp_synchronize(ctx);
}

int vp_letterbox_dev(vp_ctx* ctx, const uint8_t* src, int w, int h, int dw, int dh, int pad, float* dst, float* geom_out)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(check_lb(ctx, src, dst, w, h, dw, dh, pad));
    return vpk_letterbox(ctx, src, w, h, dw, dh, pad, dst, geom_out);
}

int vp_nms_f32(vp_ctx* ctx, const float* boxes, const float* scores, int n, float thr, int rotated, int max_keep, int32_t* keep_out,
               int32_t* n_keep_out)
{
    VP_TRY(check_ctx(ctx));
    if (n < 0 || max_keep < 0 || !n_keep_out || (n > 0 && (!boxes || !scores)) || (max_keep > 0 && !keep_out))
        return vp_fail(ctx, VP_ERR_INVALID, "vp_nms_f32 arguments");
    *n_keep_out = 0;
    if (n == 0 || max_keep == 0) return VP_OK;
    const int bs = rotated ? 5 : 4;
    vp_ws_frame W;
    float* d_boxes; W.want(&d_boxes, (size_t)n * bs * 4);
    float* d_scores; W.want(&d_scores, (size_t)n * 4);
    int* d_keep; W.want(&d_keep, (size_t)max_keep * 4);
    int* d_nk; W.want(&d_nk, 4);
    vp_nms_ws nw;
    vp_nms_want(W, n, &nw);
    VP_TRY(vp_ws_commit(ctx, W, "vp_nms_f32"));
    VP_TRY(h2d(ctx, d_boxes, boxes, (size_t)n * bs * 4));
    VP_TRY(h2d(ctx, d_scores, scores, (size_t)n * 4));
    VP_TRY(vpk_nms(ctx, d_boxes, d_scores, n, thr, rotated ? 1 : 0, max_keep, d_keep, d_nk, nw));
    VP_TRY(d2h(ctx, n_keep_out, d_nk, 4));
    VP_TRY(vp_synchronize(ctx));
    if (*n_keep_out > 0) { VP_TRY(d2h(ctx, keep_out, d_keep, (size_t)*n_keep_out * 4)); VP_TRY(vp_synchronize(ctx)); }
    return VP_OK;
}

int vp_nms_dev(vp_ctx* ctx, const float* boxes, const float* scores, int n, float thr, int rotated, int max_keep, int32_t* keep_out,
               int32_t* n_keep)
{
    VP_TRY(check_ctx(ctx));
    if (n < 0 || max_keep <= 0 || !n_keep || !keep_out || (n > 0 && (!boxes || !scores))) return vp_fail(ctx, VP_ERR_INVALID, "vp_nms_dev arguments");
    vp_ws_frame W;
    vp_nms_ws nw;
    vp_nms_want(W, n, &nw);
    VP_TRY(vp_ws_commit(ctx, W, "vp_nms_dev"));
    return vpk_nms(ctx, boxes, scores, n, thr, rotated ? 1 : 0, max_keep, keep_out, n_keep, nw);
}

// ---- element-wise operators on device images (kernels: vp_elementwise.hip) ----------------------------------------------------------
#define VP_EW_MAX ((size_t)1 << 40)
// dst is a source itself or apart from it
static bool ew_dst_ok(const void* src, const void* dst, size_t n) { return !src || src == dst || !dev_overlap(src, n, dst, n); }

int vp_bitwise_u8_dev(vp_ctx* ctx, int op, const uint8_t* d_a, const uint8_t* d_b, int scalar, const uint8_t* d_mask, int cn, size_t n, uint8_t* d_dst, int bits_w,
                      unsigned long long* d_bits, int* made_bits)
{
    VP_TRY(check_ctx(ctx));
    if (made_bits) *made_bits = 0;
    if (op < VP_BITWISE_AND || op > VP_BITWISE_NOT || !d_a || !d_dst || n == 0 || n > VP_EW_MAX || cn < 1 || cn > 4 || n % (size_t)cn != 0 ||
        (op != VP_BITWISE_NOT && !d_b && (scalar < 0 || scalar > 255)) || bits_w < 0 || (d_bits && bits_w > 0 && (cn != 1 || n % (size_t)bits_w != 0)))
        return vp_fail(ctx, VP_ERR_INVALID, "vp_bitwise_u8_dev arguments");
    if (op == VP_BITWISE_NOT) d_b = nullptr;
    if (!ew_dst_ok(d_a, d_dst, n) || !ew_dst_ok(d_b, d_dst, n) || (d_mask && dev_overlap(d_mask, n / cn, d_dst, n)) ||
        (d_bits && bits_w > 0 && (dev_overlap(d_bits, (n + 7) / 8, d_dst, n) || dev_overlap(d_bits, (n + 7) / 8, d_a, n) || (d_b && dev_overlap(d_bits, (n + 7) / 8, d_b, n)))))
        return vp_fail(ctx, VP_ERR_INVALID, "vp_bitwise_u8_dev: dst overlaps a source partly, or the mask or the bit plane overlaps an image");
    return vpk_bitwise_u8(ctx, op, d_a, d_b, scalar, d_mask, cn, n, d_dst, bits_w, reinterpret_cast<u64*>(d_bits), made_bits);
}

int vp_arith_u8_dev(vp_ctx* ctx, int op, const uint8_t* d_a, const uint8_t* d_b, size_t n, uint8_t* d_dst)
{
    VP_TRY(check_ctx(ctx));
    if (op < VP_ARITH_ADD || op > VP_ARITH_ABSDIFF || !d_a || !d_b || !d_dst || n == 0 || n > VP_EW_MAX || !ew_dst_ok(d_a, d_dst, n) || !ew_dst_ok(d_b, d_dst, n))
        return vp_fail(ctx, VP_ERR_INVALID, "vp_arith_u8_dev arguments");
    return vpk_arith_u8(ctx, op, d_a, d_b, n, d_dst);
}

int vp_lut_u8_dev(vp_ctx* ctx, const uint8_t* d_src, size_t n, int cn, const uint8_t* lut, uint8_t* d_dst)
{
    VP_TRY(check_ctx(ctx));
    if (!d_src || !d_dst || !lut || n == 0 || n > VP_EW_MAX || cn < 1 || cn > 4 || n % (size_t)cn != 0 || !ew_dst_ok(d_src, d_dst, n))
        return vp_fail(ctx, VP_ERR_INVALID, "vp_lut_u8_dev arguments");
    return vpk_lut_u8(ctx, d_src, n, cn, lut, d_dst);
}

int vp_split_u8_dev(vp_ctx* ctx, const uint8_t* d_src, size_t npx, int cn, uint8_t* d_p0, uint8_t* d_p1, uint8_t* d_p2, uint8_t* d_p3)
{
    VP_TRY(check_ctx(ctx));
    if (!d_src || npx == 0 || npx > VP_EW_MAX || cn < 2 || cn > 4) return vp_fail(ctx, VP_ERR_INVALID, "vp_split_u8_dev arguments");
    uint8_t* pl[4] = {d_p0, cn > 1 ? d_p1 : nullptr, cn > 2 ? d_p2 : nullptr, cn > 3 ? d_p3 : nullptr};
    bool any = false;
    for (int c = 0; c < cn; c++) {
        if (!pl[c]) continue;
        any = true;
        if (dev_overlap(d_src, npx * cn, pl[c], npx)) return vp_fail(ctx, VP_ERR_INVALID, "vp_split_u8_dev: a plane overlaps the source");
        for (int e = 0; e < c; e++)
            if (pl[e] && dev_overlap(pl[e], npx, pl[c], npx)) return vp_fail(ctx, VP_ERR_INVALID, "vp_split_u8_dev: planes overlap");
    }
    if (!any) return vp_fail(ctx, VP_ERR_INVALID, "vp_split_u8_dev: no destination plane");
    return vpk_split_u8(ctx, d_src, npx, cn, pl[0], pl[1], pl[2], pl[3]);
}

int vp_merge_u8_dev(vp_ctx* ctx, const uint8_t* d_p0, const uint8_t* d_p1, const uint8_t* d_p2, const uint8_t* d_p3, size_t npx, int cn, uint8_t* d_dst)
{
    VP_TRY(check_ctx(ctx));
    if (!d_dst || npx == 0 || npx > VP_EW_MAX || cn < 2 || cn > 4) return vp_fail(ctx, VP_ERR_INVALID, "vp_merge_u8_dev arguments");
    const uint8_t* pl[4] = {d_p0, d_p1, cn > 2 ? d_p2 : nullptr, cn > 3 ? d_p3 : nullptr};
    for (int c = 0; c < cn; c++)
        if (!pl[c] || dev_overlap(pl[c], npx, d_dst, npx * cn)) return vp_fail(ctx, VP_ERR_INVALID, "vp_merge_u8_dev: a plane is missing or overlaps the destination");
    return vpk_merge_u8(ctx, pl[0], pl[1], pl[2], pl[3], npx, cn, d_dst);
}

// the counter lives in the context's workspace: carved, zeroed, counted into and read back in stream order, and the call returns only
// after the read - a second call finds nothing of the first
int vp_count_nonzero_u8_dev(vp_ctx* ctx, const uint8_t* d_src, size_t n, uint64_t* count)
{
    VP_TRY(check_ctx(ctx));
    if (!d_src || !count || n == 0 || n > VP_EW_MAX) return vp_fail(ctx, VP_ERR_INVALID, "vp_count_nonzero_u8_dev arguments");
    vp_ws_frame W;
    u64* d_total; W.want(&d_total, 8);
    VP_TRY(vp_ws_commit(ctx, W, "vp_count_nonzero_u8_dev"));
    VP_TRY(vpk_count_nonzero_u8(ctx, d_src, n, d_total));
    VP_TRY(d2h(ctx, count, d_total, 8));
    return vp_synchronize(ctx);
}

}  // extern "C"
