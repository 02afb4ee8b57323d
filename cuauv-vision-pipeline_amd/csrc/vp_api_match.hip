// C ABI of libvp.so, template matching: cv2.matchTemplate on host and device images (kernels: vp_match.hip; checks, geometry and the
// workspace layout: vp_match_plan.h).
#include "vp_api_util.h"
#include "vp_match_plan.h"

extern "C" {

int vp_match_template_u8(vp_ctx* ctx, const uint8_t* src, int w, int h, int cn, const uint8_t* templ, int tw, int th, int method, float* dst)
{
    if (!src || !templ || !dst) return vp_fail(ctx, VP_ERR_INVALID, "vp_match_template_u8: a pointer is missing");
    const size_t row = w > 0 && cn > 0 ? (size_t)w * cn : 0, trow = tw > 0 && cn > 0 ? (size_t)tw * cn : 0, drow = w >= tw && w > 0 ? (size_t)(w - tw + 1) * 4 : 0;
    if (const char* why = vp_match_template_refusal(w, h, cn, row, tw, th, trow, method, drow)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    vp_match_plan P;
    vp_match_make_plan(w, h, cn, tw, th, method, &P);
    const size_t pitch = (row + 3) / 4 * 4;              // rows on word boundaries: the correlation stages them a word at a time
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, pitch * h);
    uint8_t* d_templ; W.want(&d_templ, trow * th);
    float* d_dst; W.want(&d_dst, drow * P.rh);
    uint8_t* d_ws; W.want(&d_ws, P.ws_bytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_match_template_u8"));
    VP_TRY(h2d_rows(ctx, d_src, pitch, src, row, row, h));
    VP_TRY(h2d(ctx, d_templ, templ, trow * th));
    VP_TRY(vpk_match_template(ctx, d_src, pitch, w, h, cn, d_templ, trow, tw, th, method, P, d_ws, d_dst, drow));
    VP_TRY(d2h(ctx, dst, d_dst, drow * P.rh));
    return vp_synchronize(ctx);
}

int vp_match_template_dev(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int cn, const uint8_t* d_templ, size_t templ_stride, int tw, int th,
                          int method, float* d_dst, size_t dst_stride)
{
    if (!d_src || !d_templ || !d_dst) return vp_fail(ctx, VP_ERR_INVALID, "vp_match_template_dev: a pointer is missing");
    if (const char* why = vp_match_template_refusal(w, h, cn, stride, tw, th, templ_stride, method, dst_stride)) return vp_fail(ctx, VP_ERR_INVALID, why);
    const size_t dbytes = strided_bytes(dst_stride, (size_t)(w - tw + 1) * 4, h - th + 1);
    if ((uintptr_t)d_dst % 4 || dev_overlap(d_src, strided_bytes(stride, (size_t)w * cn, h), d_dst, dbytes) ||
        dev_overlap(d_templ, strided_bytes(templ_stride, (size_t)tw * cn, th), d_dst, dbytes))
        return vp_fail(ctx, VP_ERR_INVALID, "vp_match_template_dev: dst is not 4-byte aligned, or overlaps the image or the template");
    VP_TRY(check_ctx(ctx));
    vp_match_plan P;
    vp_match_make_plan(w, h, cn, tw, th, method, &P);
    vp_ws_frame W;
    uint8_t* d_ws; W.want(&d_ws, P.ws_bytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_match_template_dev"));
    return vpk_match_template(ctx, d_src, stride, w, h, cn, d_templ, templ_stride, tw, th, method, P, d_ws, d_dst, dst_stride);
}

}  // extern "C"
