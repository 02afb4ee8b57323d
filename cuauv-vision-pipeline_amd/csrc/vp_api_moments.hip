// C ABI of libvp.so, moments: the raster and per-label sums of host and device images (kernels: vp_moments), and the two host-only
// pieces of cv2.moments that are double arithmetic in a fixed order - a contour's Green sums and completeMomentState.
#include "vp_api_util.h"
#include "vp_moments_plan.h"
#include <float.h>

// the table (d_out: ten words; d_table: label_table_bytes) lives in the caller's frame: zeroed, added into and read back in stream
// order; the call returns after the read
static int moments_run(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int binary, const u64* d_bits, u64* d_out, uint64_t* out10)
{
    VP_TRY(vpk_moments_u8(ctx, d_src, stride, w, h, binary, d_bits, d_out));
    VP_TRY(d2h(ctx, out10, d_out, 10 * sizeof(u64)));
    return vp_synchronize(ctx);
}

static size_t label_table_bytes(int nlabels) { return (size_t)nlabels * 10 * sizeof(u64); }
static int label_moments_run(vp_ctx* ctx, const int32_t* d_labels, size_t stride, int w, int h, int nlabels, u64* d_table, uint64_t* out)
{
    const size_t bytes = label_table_bytes(nlabels);
    VP_TRY(vpk_label_moments_i32(ctx, d_labels, stride, w, h, nlabels, d_table));
    VP_TRY(d2h(ctx, out, d_table, bytes));
    return vp_synchronize(ctx);
}

static const char* label_refusal(const int32_t* labels, size_t stride, int w, int h, int nlabels, const uint64_t* out)
{
    if (!labels || !out) return "label moments: a pointer is missing";
    if (nlabels < 1) return "label moments: nlabels must be at least 1";
    if (const char* why = vp_moments_refusal(w, h, stride, 4, 1)) return why;
    if (stride % 4 || (uintptr_t)labels % 4) return "label moments: rows of int32 must be 4-byte aligned";
    return nullptr;
}

extern "C" {

int vp_moments_u8(vp_ctx* ctx, const uint8_t* src, size_t stride, int w, int h, int binary, uint64_t* out10)
{
    if (!src || !out10) return vp_fail(ctx, VP_ERR_INVALID, "vp_moments_u8: a pointer is missing");
    if (const char* why = vp_moments_refusal(w, h, stride, 1, binary ? 1 : 255)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    const size_t npx = (size_t)w * h;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, npx);
    u64* d_out; W.want(&d_out, 10 * sizeof(u64));
    VP_TRY(vp_ws_commit(ctx, W, "vp_moments_u8"));
    VP_TRY(h2d_rows(ctx, d_src, (size_t)w, src, stride, (size_t)w, h));
    return moments_run(ctx, d_src, (size_t)w, w, h, binary != 0, nullptr, d_out, out10);
}

int vp_moments_dev(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int binary, const unsigned long long* d_bits, uint64_t* out10)
{
    if ((!d_src && !d_bits) || !out10) return vp_fail(ctx, VP_ERR_INVALID, "vp_moments_dev: a pointer is missing");
    if (d_bits && !binary) return vp_fail(ctx, VP_ERR_INVALID, "vp_moments_dev: a bit plane gives binary moments only");
    if (d_bits && (uintptr_t)d_bits % 8) return vp_fail(ctx, VP_ERR_INVALID, "vp_moments_dev: the bit plane must be 8-byte aligned");
    if (const char* why = vp_moments_refusal(w, h, d_bits ? (size_t)w : stride, 1, binary ? 1 : 255)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    vp_ws_frame W;
    u64* d_out; W.want(&d_out, 10 * sizeof(u64));
    VP_TRY(vp_ws_commit(ctx, W, "vp_moments_dev"));
    return moments_run(ctx, d_src, stride, w, h, binary != 0, reinterpret_cast<const u64*>(d_bits), d_out, out10);
}

int vp_label_moments_i32(vp_ctx* ctx, const int32_t* labels, size_t stride, int w, int h, int nlabels, uint64_t* out)
{
    if (const char* why = label_refusal(labels, stride, w, h, nlabels, out)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    const size_t bytes = (size_t)w * h * 4;
    vp_ws_frame W;
    int32_t* d_labels; W.want(&d_labels, bytes);
    u64* d_table; W.want(&d_table, label_table_bytes(nlabels));
    VP_TRY(vp_ws_commit(ctx, W, "vp_label_moments_i32"));
    VP_TRY(h2d_rows(ctx, d_labels, (size_t)w * 4, labels, stride, (size_t)w * 4, h));
    return label_moments_run(ctx, d_labels, (size_t)w * 4, w, h, nlabels, d_table, out);
}

int vp_label_moments_dev(vp_ctx* ctx, const int32_t* d_labels, size_t stride, int w, int h, int nlabels, uint64_t* out)
{
    if (const char* why = label_refusal(d_labels, stride, w, h, nlabels, out)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    vp_ws_frame W;
    u64* d_table; W.want(&d_table, label_table_bytes(nlabels));
    VP_TRY(vp_ws_commit(ctx, W, "vp_label_moments_dev"));
    return label_moments_run(ctx, d_labels, stride, w, h, nlabels, d_table, out);
}

// imgproc/src/moments.cpp contourMoments: Green's theorem in float64, from the last point round, in this operation order - the sums
// of the higher orders pass 2^53, so the order is the result.
int vp_polygon_moments(const void* pts, int is_float32, int n, double* out10)
{
    if (!out10 || n < 0 || (n > 0 && !pts)) return VP_ERR_INVALID;
    for (int k = 0; k < 10; k++) out10[k] = 0.0;
    if (n == 0) return VP_OK;
    const int32_t* pi = static_cast<const int32_t*>(pts);
    const float* pf = static_cast<const float*>(pts);
    double a00 = 0, a10 = 0, a01 = 0, a20 = 0, a11 = 0, a02 = 0, a30 = 0, a21 = 0, a12 = 0, a03 = 0;
    double xi_1 = is_float32 ? (double)pf[2 * (n - 1)] : (double)pi[2 * (n - 1)];
    double yi_1 = is_float32 ? (double)pf[2 * (n - 1) + 1] : (double)pi[2 * (n - 1) + 1];
    double xi_12 = xi_1 * xi_1, yi_12 = yi_1 * yi_1;
    for (int i = 0; i < n; i++) {
        const double xi = is_float32 ? (double)pf[2 * i] : (double)pi[2 * i];
        const double yi = is_float32 ? (double)pf[2 * i + 1] : (double)pi[2 * i + 1];
        const double xi2 = xi * xi, yi2 = yi * yi;
        const double dxy = xi_1 * yi - xi * yi_1;
        const double xii_1 = xi_1 + xi, yii_1 = yi_1 + yi;
        a00 += dxy;
        a10 += dxy * xii_1;
        a01 += dxy * yii_1;
        a20 += dxy * (xi_1 * xii_1 + xi2);
        a11 += dxy * (xi_1 * (yii_1 + yi_1) + xi * (yii_1 + yi));
        a02 += dxy * (yi_1 * yii_1 + yi2);
        a30 += dxy * xii_1 * (xi_12 + xi2);
        a03 += dxy * yii_1 * (yi_12 + yi2);
        a21 += dxy * (xi_12 * (3 * yi_1 + yi) + 2 * xi * xi_1 * yii_1 + xi2 * (yi_1 + 3 * yi));
        a12 += dxy * (yi_12 * (3 * xi_1 + xi) + 2 * yi * yi_1 * xii_1 + yi2 * (xi_1 + 3 * xi));
        xi_1 = xi; yi_1 = yi; xi_12 = xi2; yi_12 = yi2;
    }
    if (fabs(a00) > FLT_EPSILON) {
        const double sg = a00 > 0 ? 1.0 : -1.0;
        const double db1_2 = sg * 0.5, db1_6 = sg * (1.0 / 6), db1_12 = sg * (1.0 / 12), db1_24 = sg * (1.0 / 24), db1_20 = sg * (1.0 / 20),
                     db1_60 = sg * (1.0 / 60);
        out10[0] = a00 * db1_2;
        out10[1] = a10 * db1_6;
        out10[2] = a01 * db1_6;
        out10[3] = a20 * db1_12;
        out10[4] = a11 * db1_24;
        out10[5] = a02 * db1_12;
        out10[6] = a30 * db1_20;
        out10[7] = a21 * db1_60;
        out10[8] = a12 * db1_60;
        out10[9] = a03 * db1_20;
    }
    return VP_OK;
}

// completeMomentState: centre, central moments, normalised central moments
int vp_moments_complete(const double* m, double* out24)
{
    if (!m || !out24) return VP_ERR_INVALID;
    const double m00 = m[0], m10 = m[1], m01 = m[2], m20 = m[3], m11 = m[4], m02 = m[5], m30 = m[6], m21 = m[7], m12 = m[8], m03 = m[9];
    double cx = 0, cy = 0, inv_m00 = 0;
    if (fabs(m00) > DBL_EPSILON) {
        inv_m00 = 1. / m00;
        cx = m10 * inv_m00;
        cy = m01 * inv_m00;
    }
    const double mu20 = m20 - m10 * cx;
    const double mu11 = m11 - m10 * cy;
    const double mu02 = m02 - m01 * cy;
    const double mu30 = m30 - cx * (3 * mu20 + cx * m10);
    const double mu21 = m21 - cx * (2 * mu11 + cx * m01) - cy * mu20;
    const double mu12 = m12 - cy * (2 * mu11 + cy * m10) - cx * mu02;
    const double mu03 = m03 - cy * (3 * mu02 + cy * m01);
    const double s2 = inv_m00 * inv_m00, s3 = s2 * sqrt(fabs(inv_m00));
    for (int k = 0; k < 10; k++) out24[k] = m[k];
    const double mu[7] = {mu20, mu11, mu02, mu30, mu21, mu12, mu03};
    for (int k = 0; k < 7; k++) out24[10 + k] = mu[k];
    for (int k = 0; k < 3; k++) out24[17 + k] = mu[k] * s2;
    for (int k = 3; k < 7; k++) out24[17 + k] = mu[k] * s3;
    return VP_OK;
}

}  // extern "C"
