// C ABI of libvp.so, stereo block matching: disparity of a rectified pair and metric depth on host and device images (kernels:
// vp_stereo.hip; checks, geometry and the shared formulas: vp_stereo_plan.h), and the same statement as plain scalar C++.
#include "vp_api_util.h"
#include "vp_stereo_plan.h"

int vpk_stereo_bm(vp_ctx* ctx, const uint8_t* d_left, size_t lstride, const uint8_t* d_right, size_t rstride, int w, int h, int nd, int min_disp, int cap, int texture,
                  int uniq, const vp_stereo_plan& P, uint8_t* d_ws, int16_t* d_disp, size_t dstride);
int vpk_stereo_depth(vp_ctx* ctx, const int16_t* d_disp, size_t sstride, int w, int h, double fb, float* d_depth, size_t dstride);

// everything the three matcher entries refuse, from the arguments alone
static const char* bm_check(const uint8_t* left, size_t lstride, const uint8_t* right, size_t rstride, int w, int h, int nd, int block, int min_disp, int cap, int texture,
                            int uniq, const int16_t* disp, size_t dstride)
{
    if (!left || !right || !disp) return "stereo: a pointer is missing";
    if (const char* why = vp_stereo_bm_refusal(w, h, lstride, rstride, nd, block, min_disp, cap, texture, uniq, dstride)) return why;
    if ((uintptr_t)disp % 2) return "stereo: the result is not aligned to its element size";
    const size_t dbytes = strided_bytes(dstride, (size_t)w * 2, h);
    if (dev_overlap(left, strided_bytes(lstride, w, h), disp, dbytes) || dev_overlap(right, strided_bytes(rstride, w, h), disp, dbytes))
        return "stereo: the result overlaps an input image";
    return nullptr;
}

static const char* depth_check(const int16_t* disp, size_t sstride, int w, int h, const float* depth, size_t dstride)
{
    if (!disp || !depth) return "depth: a pointer is missing";
    if (const char* why = vp_depth_refusal(w, h, sstride, dstride)) return why;
    if ((uintptr_t)disp % 2 || (uintptr_t)depth % 4) return "depth: an image is not aligned to its element size";
    if (dev_overlap(disp, strided_bytes(sstride, (size_t)w * 2, h), depth, strided_bytes(dstride, (size_t)w * 4, h))) return "depth: the result overlaps the disparity";
    return nullptr;
}

extern "C" {

int vp_stereo_bm_plan(int w, int h, int num_disparities, int block_size, int min_disparity, int32_t* rect, size_t* ws_bytes, int32_t* geometry)
{
    if (!rect || !ws_bytes || !geometry) return vp_fail(nullptr, VP_ERR_INVALID, "vp_stereo_bm_plan: a pointer is missing");
    if (const char* why = vp_stereo_geometry_refusal(w, h, num_disparities, block_size, min_disparity)) return vp_fail(nullptr, VP_ERR_INVALID, why);
    vp_stereo_plan P;
    vp_stereo_make_plan(w, h, num_disparities, block_size, min_disparity, &P);
    rect[0] = P.cw ? P.cx0 : 0;
    rect[1] = P.cw ? P.cy0 : 0;
    rect[2] = P.cw;
    rect[3] = P.ch;
    *ws_bytes = P.ws_bytes;
    geometry[0] = P.strip_cols;
    geometry[1] = P.band_rows;
    geometry[2] = (int32_t)P.grid_x;
    geometry[3] = (int32_t)P.grid_y;
    geometry[4] = (int32_t)P.lds_bytes;
    return VP_OK;
}

int vp_stereo_bm_dev(vp_ctx* ctx, const uint8_t* left_dev, size_t left_stride, const uint8_t* right_dev, size_t right_stride, int w, int h, int num_disparities,
                     int block_size, int min_disparity, int pre_filter_cap, int texture_threshold, int uniqueness_ratio, int16_t* disp_dev, size_t disp_stride)
{
    if (const char* why = bm_check(left_dev, left_stride, right_dev, right_stride, w, h, num_disparities, block_size, min_disparity, pre_filter_cap, texture_threshold,
                                   uniqueness_ratio, disp_dev, disp_stride))
        return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    vp_stereo_plan P;
    vp_stereo_make_plan(w, h, num_disparities, block_size, min_disparity, &P);
    vp_ws_frame W;
    uint8_t* d_ws; W.want(&d_ws, P.ws_bytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_stereo_bm_dev"));
    return vpk_stereo_bm(ctx, left_dev, left_stride, right_dev, right_stride, w, h, num_disparities, min_disparity, pre_filter_cap, texture_threshold, uniqueness_ratio, P,
                         d_ws, disp_dev, disp_stride);
}

int vp_stereo_bm_u8(vp_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, int num_disparities, int block_size, int min_disparity, int pre_filter_cap,
                    int texture_threshold, int uniqueness_ratio, int16_t* disp)
{
    const size_t row = w > 0 ? (size_t)w : 0;
    if (const char* why = bm_check(left, row, right, row, w, h, num_disparities, block_size, min_disparity, pre_filter_cap, texture_threshold, uniqueness_ratio, disp, row * 2))
        return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    vp_stereo_plan P;
    vp_stereo_make_plan(w, h, num_disparities, block_size, min_disparity, &P);
    vp_ws_frame W;
    uint8_t* d_left; W.want(&d_left, row * h);
    uint8_t* d_right; W.want(&d_right, row * h);
    int16_t* d_disp; W.want(&d_disp, row * 2 * h);
    uint8_t* d_ws; W.want(&d_ws, P.ws_bytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_stereo_bm_u8"));
    VP_TRY(h2d(ctx, d_left, left, row * h));
    VP_TRY(h2d(ctx, d_right, right, row * h));
    VP_TRY(vpk_stereo_bm(ctx, d_left, row, d_right, row, w, h, num_disparities, min_disparity, pre_filter_cap, texture_threshold, uniqueness_ratio, P, d_ws, d_disp, row * 2));
    VP_TRY(d2h(ctx, disp, d_disp, row * 2 * h));
    return vp_synchronize(ctx);
}

int vp_stereo_bm_host(const uint8_t* left, size_t left_stride, const uint8_t* right, size_t right_stride, int w, int h, int num_disparities, int block_size,
                      int min_disparity, int pre_filter_cap, int texture_threshold, int uniqueness_ratio, int16_t* disp, size_t disp_stride)
{
    if (const char* why = bm_check(left, left_stride, right, right_stride, w, h, num_disparities, block_size, min_disparity, pre_filter_cap, texture_threshold,
                                   uniqueness_ratio, disp, disp_stride))
        return vp_fail(nullptr, VP_ERR_INVALID, why);
    vp_stereo_plan P;
    vp_stereo_make_plan(w, h, num_disparities, block_size, min_disparity, &P);
    const int nd = num_disparities, r = P.r, cap = pre_filter_cap, inv = vp_stereo_invalid(min_disparity);
    const size_t dpitch = disp_stride / 2;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) disp[(size_t)y * dpitch + x] = (int16_t)inv;
    if (!P.cw) return VP_OK;
    std::vector<uint8_t> pl((size_t)w * h), pr((size_t)w * h);
    vp_stereo_host_prefilter(left, left_stride, w, h, cap, pl.data());
    vp_stereo_host_prefilter(right, right_stride, w, h, cap, pr.data());
    // vertical sums over the window's rows, per disparity and column of [vx0, vx0 + vn); then one row of window sums
    const int vx0 = P.cx0 - r, vn = P.cw + 2 * r;
    std::vector<int32_t> V((size_t)nd * vn, 0), tex(vn, 0), C((size_t)nd * P.cw);
    auto add_row = [&](int y, int sign) {
        const uint8_t *lrow = pl.data() + (size_t)y * w, *rrow = pr.data() + (size_t)y * w;
        for (int d = 0; d < nd; d++) {
            const int D = min_disparity + d;
            int32_t* v = V.data() + (size_t)d * vn;
            for (int i = 0; i < vn; i++) v[i] += sign * std::abs((int)lrow[vx0 + i] - (int)rrow[vx0 + i - D]);
        }
        for (int i = 0; i < vn; i++) tex[i] += sign * std::abs((int)lrow[vx0 + i] - cap);
    };
    for (int y = P.cy0 - r; y < P.cy0 + r; y++) add_row(y, 1);
    for (int y = P.cy0; y < P.cy0 + P.ch; y++) {
        add_row(y + r, 1);
        if (y > P.cy0) add_row(y - r - 1, -1);
        for (int d = 0; d < nd; d++) {
            const int32_t* v = V.data() + (size_t)d * vn;
            int32_t* c = C.data() + (size_t)d * P.cw;
            int32_t acc = 0;
            for (int k = 0; k <= 2 * r; k++) acc += v[k];
            for (int x = 0;; x++) {
                c[x] = acc;
                if (x + 1 == P.cw) break;
                acc += v[x + 2 * r + 1] - v[x];
            }
        }
        int32_t tacc = 0;
        for (int k = 0; k <= 2 * r; k++) tacc += tex[k];
        for (int x = 0; x < P.cw; x++) {
            const int32_t T = tacc;
            if (x + 1 < P.cw) tacc += tex[x + 2 * r + 1] - tex[x];
            if (T < texture_threshold) continue;
            int ds = 0, cmin = C[x];
            for (int d = 1; d < nd; d++)
                if (C[(size_t)d * P.cw + x] <= cmin) { cmin = C[(size_t)d * P.cw + x]; ds = d; }
            if (uniqueness_ratio > 0) {
                const int limit = cmin + cmin * uniqueness_ratio / 100;
                bool rival = false;
                for (int d = 0; d < nd && !rival; d++) rival = (d < ds - 1 || d > ds + 1) && C[(size_t)d * P.cw + x] <= limit;
                if (rival) continue;
            }
            const int dm = ds > 0 ? ds - 1 : ds + 1, dq = ds < nd - 1 ? ds + 1 : ds - 1;
            disp[(size_t)y * dpitch + P.cx0 + x] = vp_stereo_subpixel(cmin, C[(size_t)dm * P.cw + x], C[(size_t)dq * P.cw + x], min_disparity + ds);
        }
    }
    return VP_OK;
}

int vp_depth_from_disparity_dev(vp_ctx* ctx, const int16_t* disp_dev, size_t disp_stride, int w, int h, double focal_px, double baseline_m, float* depth_dev,
                                size_t depth_stride)
{
    if (const char* why = depth_check(disp_dev, disp_stride, w, h, depth_dev, depth_stride)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    return vpk_stereo_depth(ctx, disp_dev, disp_stride, w, h, focal_px * baseline_m, depth_dev, depth_stride);
}

int vp_depth_from_disparity_i16(vp_ctx* ctx, const int16_t* disp, int w, int h, double focal_px, double baseline_m, float* depth)
{
    const size_t n = w > 0 ? (size_t)w : 0;
    if (const char* why = depth_check(disp, n * 2, w, h, depth, n * 4)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    vp_ws_frame W;
    int16_t* d_disp; W.want(&d_disp, n * 2 * h);
    float* d_depth; W.want(&d_depth, n * 4 * h);
    VP_TRY(vp_ws_commit(ctx, W, "vp_depth_from_disparity_i16"));
    VP_TRY(h2d(ctx, d_disp, disp, n * 2 * h));
    VP_TRY(vpk_stereo_depth(ctx, d_disp, n * 2, w, h, focal_px * baseline_m, d_depth, n * 4));
    VP_TRY(d2h(ctx, depth, d_depth, n * 4 * h));
    return vp_synchronize(ctx);
}

int vp_depth_from_disparity_host(const int16_t* disp, size_t disp_stride, int w, int h, double focal_px, double baseline_m, float* depth, size_t depth_stride)
{
    if (const char* why = depth_check(disp, disp_stride, w, h, depth, depth_stride)) return vp_fail(nullptr, VP_ERR_INVALID, why);
    const double fb = focal_px * baseline_m;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) depth[(size_t)y * (depth_stride / 4) + x] = vp_stereo_depth(fb, disp[(size_t)y * (disp_stride / 2) + x]);
    return VP_OK;
}

}  // extern "C"
