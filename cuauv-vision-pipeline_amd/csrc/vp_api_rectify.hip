// C ABI of libvp.so, stereo rectification and 3-D reprojection: both eyes of a raw frame to the matcher's inputs in one launch, and
// a disparity image to XYZ points, on host and device images (kernels: vp_rectify.hip; tile, refusals and the shared formulas:
// vp_rectify_plan.h), and the same statements as plain scalar C++.
#include "vp_api_util.h"
#include "vp_rectify_plan.h"

static_assert(VP_DISP_I16 == VP_RJ_I16 && VP_DISP_F32 == VP_RJ_F32, "the plan header spells the disparity types of include/vp.h");

int vpk_rectify_pair(vp_ctx* ctx, const uint8_t* const* d_src, const size_t* sstride, int w, int h, int cn, const int16_t* const* d_xy, const uint16_t* const* d_frac,
                     int ow, int oh, uint8_t* const* d_grey, const size_t* gstride, uint8_t* const* d_colour, const size_t* cstride);
int vpk_reproject(vp_ctx* ctx, const void* d_disp, size_t dstride, int disp_type, int w, int h, const double* q16, int invalid, float* d_xyz, size_t xstride);

// the arguments of one rectify call, eye by eye (0 left, 1 right)
struct rp_call {
    const uint8_t* src[2]; size_t sstride[2];
    const int16_t* xy[2]; const uint16_t* frac[2];
    uint8_t* grey[2]; size_t gstride[2];
    uint8_t* colour[2]; size_t cstride[2];
};

// everything the rectify entries refuse, from the arguments alone
static const char* rectify_check(const rp_call& K, int w, int h, int cn, int ow, int oh)
{
    if (const char* why = vp_rectify_size_refusal(w, h, cn, ow, oh)) return why;
    struct span { const void* p; size_t n; };
    span in[6], out[4];
    int nout = 0;
    for (int e = 0; e < 2; e++) {
        if (!K.src[e]) return "rectify: a source image is missing";
        if (!K.xy[e] || !K.frac[e]) return "rectify: a table is missing";
        if (!K.grey[e]) return "rectify: a grey result is missing";
        if (K.sstride[e] < (size_t)w * cn) return "rectify: a source stride is below the row";
        if (K.gstride[e] < (size_t)ow) return "rectify: a grey result's stride is below the row";
        if (K.colour[e] && K.cstride[e] < (size_t)ow * cn) return "rectify: a colour result's stride is below the row";
        if ((uintptr_t)K.xy[e] % 2 || (uintptr_t)K.frac[e] % 2) return "rectify: a table is not aligned to its element size";
        in[3 * e] = {K.src[e], strided_bytes(K.sstride[e], (size_t)w * cn, h)};
        in[3 * e + 1] = {K.xy[e], (size_t)ow * oh * 4};
        in[3 * e + 2] = {K.frac[e], (size_t)ow * oh * 2};
        out[nout++] = {K.grey[e], strided_bytes(K.gstride[e], ow, oh)};
        if (K.colour[e]) out[nout++] = {K.colour[e], strided_bytes(K.cstride[e], (size_t)ow * cn, oh)};
    }
    for (int a = 0; a < nout; a++) {
        for (int i = 0; i < 6; i++)
            if (dev_overlap(out[a].p, out[a].n, in[i].p, in[i].n)) return "rectify: a result overlaps a source image or a table";
        for (int b = a + 1; b < nout; b++)
            if (dev_overlap(out[a].p, out[a].n, out[b].p, out[b].n)) return "rectify: two results overlap";
    }
    return nullptr;
}

static const char* reproject_check(const void* disp, size_t dstride, int disp_type, int w, int h, const double* q16, int invalid, const float* xyz, size_t xstride)
{
    if (!disp || !xyz) return "reproject: a pointer is missing";
    if (const char* why = vp_reproject_refusal(disp_type, w, h, dstride, q16, invalid, xstride)) return why;
    const size_t es = disp_type == VP_RJ_I16 ? 2 : 4;
    if ((uintptr_t)disp % es || (uintptr_t)xyz % 4) return "reproject: an image is not aligned to its element size";
    if (dev_overlap(disp, strided_bytes(dstride, (size_t)w * es, h), xyz, strided_bytes(xstride, (size_t)w * 12, h))) return "reproject: the result overlaps the disparity";
    return nullptr;
}

template <int CN>
static void rectify_host_eye(const rp_call& K, int e, int w, int h, int ow, int oh)
{
    for (int y = 0; y < oh; y++)
        for (int x = 0; x < ow; x++) {
            const size_t i = (size_t)y * ow + x;
            uint8_t o[CN];
            vp_rectify_sample<CN>(K.src[e], K.sstride[e], w, h, K.xy[e][2 * i], K.xy[e][2 * i + 1], K.frac[e][i] & 1023, o);
            K.grey[e][(size_t)y * K.gstride[e] + x] = CN == 1 ? o[0] : (uint8_t)vp_rectify_grey(o[0], o[CN > 1 ? 1 : 0], o[CN > 2 ? 2 : 0]);
            if (K.colour[e])
                for (int c = 0; c < CN; c++) K.colour[e][(size_t)y * K.cstride[e] + (size_t)x * CN + c] = o[c];
        }
}

static int reproject_staged(vp_ctx* ctx, const void* disp, int disp_type, int w, int h, const double* q16, int invalid, float* xyz, const char* who)
{
    const size_t n = w > 0 ? (size_t)w : 0, es = disp_type == VP_RJ_I16 ? 2 : 4;
    if (const char* why = reproject_check(disp, n * es, disp_type, w, h, q16, invalid, xyz, n * 12)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    vp_ws_frame W;
    uint8_t* d_disp; W.want(&d_disp, n * es * h);
    float* d_xyz; W.want(&d_xyz, n * 12 * h);
    VP_TRY(vp_ws_commit(ctx, W, who));
    VP_TRY(h2d(ctx, d_disp, disp, n * es * h));
    VP_TRY(vpk_reproject(ctx, d_disp, n * es, disp_type, w, h, q16, invalid, d_xyz, n * 12));
    VP_TRY(d2h(ctx, xyz, d_xyz, n * 12 * h));
    return vp_synchronize(ctx);
}

extern "C" {

int vp_rectify_pair_plan(int w, int h, int cn, int out_w, int out_h, int32_t* geometry)
{
    if (!geometry) return vp_fail(nullptr, VP_ERR_INVALID, "vp_rectify_pair_plan: a pointer is missing");
    if (const char* why = vp_rectify_size_refusal(w, h, cn, out_w, out_h)) return vp_fail(nullptr, VP_ERR_INVALID, why);
    geometry[0] = RP_TW;
    geometry[1] = RP_TH;
    geometry[2] = RP_PPT;
    geometry[3] = (int32_t)vp_rectify_grid_x(out_w);
    geometry[4] = (int32_t)vp_rectify_grid_y(out_h);
    geometry[5] = 2;
    return VP_OK;
}

int vp_rectify_pair_dev(vp_ctx* ctx, const uint8_t* left_dev, size_t left_stride, const uint8_t* right_dev, size_t right_stride, int w, int h, int cn,
                        const int16_t* xy_left_dev, const uint16_t* frac_left_dev, const int16_t* xy_right_dev, const uint16_t* frac_right_dev, int out_w, int out_h,
                        uint8_t* grey_left_dev, size_t grey_left_stride, uint8_t* grey_right_dev, size_t grey_right_stride, uint8_t* colour_left_dev,
                        size_t colour_left_stride, uint8_t* colour_right_dev, size_t colour_right_stride)
{
    const rp_call K = {{left_dev, right_dev}, {left_stride, right_stride}, {xy_left_dev, xy_right_dev}, {frac_left_dev, frac_right_dev},
                       {grey_left_dev, grey_right_dev}, {grey_left_stride, grey_right_stride}, {colour_left_dev, colour_right_dev}, {colour_left_stride, colour_right_stride}};
    if (const char* why = rectify_check(K, w, h, cn, out_w, out_h)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    return vpk_rectify_pair(ctx, K.src, K.sstride, w, h, cn, K.xy, K.frac, out_w, out_h, K.grey, K.gstride, K.colour, K.cstride);
}

int vp_rectify_pair_u8(vp_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, int cn, const int16_t* xy_left, const uint16_t* frac_left,
                       const int16_t* xy_right, const uint16_t* frac_right, int out_w, int out_h, uint8_t* grey_left, uint8_t* grey_right, uint8_t* colour_left,
                       uint8_t* colour_right)
{
    const size_t srow = (w > 0 && cn > 0) ? (size_t)w * cn : 0, grow = out_w > 0 ? (size_t)out_w : 0, crow = cn > 0 ? grow * cn : 0;
    const rp_call K = {{left, right}, {srow, srow}, {xy_left, xy_right}, {frac_left, frac_right}, {grey_left, grey_right}, {grow, grow}, {colour_left, colour_right}, {crow, crow}};
    if (const char* why = rectify_check(K, w, h, cn, out_w, out_h)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    const size_t sbytes = srow * h, entries = grow * out_h;
    rp_call D = K;
    vp_ws_frame W;
    uint8_t* d_src[2]; int16_t* d_xy[2]; uint16_t* d_frac[2]; uint8_t* d_grey[2]; uint8_t* d_col[2] = {nullptr, nullptr};
    for (int e = 0; e < 2; e++) {
        W.want(&d_src[e], sbytes);
        W.want(&d_xy[e], entries * 4);
        W.want(&d_frac[e], entries * 2);
        W.want(&d_grey[e], entries);
        if (K.colour[e]) W.want(&d_col[e], entries * cn);
    }
    VP_TRY(vp_ws_commit(ctx, W, "vp_rectify_pair_u8"));
    for (int e = 0; e < 2; e++) {
        VP_TRY(h2d(ctx, d_src[e], K.src[e], sbytes));
        VP_TRY(h2d(ctx, d_xy[e], K.xy[e], entries * 4));
        VP_TRY(h2d(ctx, d_frac[e], K.frac[e], entries * 2));
        D.src[e] = d_src[e]; D.xy[e] = d_xy[e]; D.frac[e] = d_frac[e]; D.grey[e] = d_grey[e]; D.colour[e] = d_col[e];
    }
    VP_TRY(vpk_rectify_pair(ctx, D.src, D.sstride, w, h, cn, D.xy, D.frac, out_w, out_h, D.grey, D.gstride, D.colour, D.cstride));
    for (int e = 0; e < 2; e++) {
        VP_TRY(d2h(ctx, K.grey[e], d_grey[e], entries));
        if (K.colour[e]) VP_TRY(d2h(ctx, K.colour[e], d_col[e], entries * cn));
    }
    return vp_synchronize(ctx);
}

int vp_rectify_pair_host(const uint8_t* left, size_t left_stride, const uint8_t* right, size_t right_stride, int w, int h, int cn, const int16_t* xy_left,
                         const uint16_t* frac_left, const int16_t* xy_right, const uint16_t* frac_right, int out_w, int out_h, uint8_t* grey_left, size_t grey_left_stride,
                         uint8_t* grey_right, size_t grey_right_stride, uint8_t* colour_left, size_t colour_left_stride, uint8_t* colour_right, size_t colour_right_stride)
{
    const rp_call K = {{left, right}, {left_stride, right_stride}, {xy_left, xy_right}, {frac_left, frac_right}, {grey_left, grey_right},
                       {grey_left_stride, grey_right_stride}, {colour_left, colour_right}, {colour_left_stride, colour_right_stride}};
    if (const char* why = rectify_check(K, w, h, cn, out_w, out_h)) return vp_fail(nullptr, VP_ERR_INVALID, why);
    for (int e = 0; e < 2; e++) {
        if (cn == 1) rectify_host_eye<1>(K, e, w, h, out_w, out_h);
        else if (cn == 3) rectify_host_eye<3>(K, e, w, h, out_w, out_h);
        else rectify_host_eye<4>(K, e, w, h, out_w, out_h);
    }
    return VP_OK;
}

int vp_reproject_to_3d_dev(vp_ctx* ctx, const void* disp_dev, size_t disp_stride, int disp_type, int w, int h, const double* q16, int invalid_disp, float* xyz_dev,
                           size_t xyz_stride)
{
    if (const char* why = reproject_check(disp_dev, disp_stride, disp_type, w, h, q16, invalid_disp, xyz_dev, xyz_stride)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    return vpk_reproject(ctx, disp_dev, disp_stride, disp_type, w, h, q16, invalid_disp, xyz_dev, xyz_stride);
}

int vp_reproject_to_3d_i16(vp_ctx* ctx, const int16_t* disp, int w, int h, const double* q16, int invalid_disp, float* xyz)
{
    return reproject_staged(ctx, disp, VP_RJ_I16, w, h, q16, invalid_disp, xyz, "vp_reproject_to_3d_i16");
}

int vp_reproject_to_3d_f32(vp_ctx* ctx, const float* disp, int w, int h, const double* q16, float* xyz)
{
    return reproject_staged(ctx, disp, VP_RJ_F32, w, h, q16, INT_MIN, xyz, "vp_reproject_to_3d_f32");
}

int vp_reproject_to_3d_host(const void* disp, size_t disp_stride, int disp_type, int w, int h, const double* q16, int invalid_disp, float* xyz, size_t xyz_stride)
{
    if (const char* why = reproject_check(disp, disp_stride, disp_type, w, h, q16, invalid_disp, xyz, xyz_stride)) return vp_fail(nullptr, VP_ERR_INVALID, why);
    for (int y = 0; y < h; y++) {
        const uint8_t* row = (const uint8_t*)disp + (size_t)y * disp_stride;
        float* out = xyz + (size_t)y * (xyz_stride / 4);
        for (int x = 0; x < w; x++) {
            if (disp_type == VP_RJ_I16) vp_reproject_i16(q16, x, y, ((const int16_t*)row)[x], invalid_disp, out + 3 * x);
            else vp_reproject_f32(q16, x, y, ((const float*)row)[x], out + 3 * x);
        }
    }
    return VP_OK;
}

}  // extern "C"
