// C ABI of libvp.so, distances: cv2.distanceTransform (DIST_L2 precise, DIST_L1, DIST_C) and cv2.minMaxLoc on host and device images
// (kernels: vp_dist.hip; checks, geometry and the search keys: vp_dist_plan.h).
#include "vp_api_util.h"
#include "vp_dist_plan.h"

// the search on the device, its two words (d_keys: 16 bytes of workspace) back through pinned staging, decoded into *out
static int min_max_loc_run(vp_ctx* ctx, const void* d_src, size_t stride, int w, int h, int depth, const uint8_t* d_mask, size_t mstride, const u64* d_bits,
                           u64* d_keys, vp_min_max_loc_result* out)
{
    VP_TRY(vpk_min_max_loc(ctx, d_src, stride, w, h, depth, d_mask, mstride, d_bits, d_keys));
    u64* hk = (u64*)vp_hstage(ctx, 16);
    if (!hk) return vp_fail(ctx, VP_ERR_NOMEM, "pinned staging");
    VP_TRY(d2h(ctx, hk, d_keys, 16));
    VP_TRY(vp_synchronize(ctx));
    vp_min_max_loc_decode(hk[0], hk[1], w, out);
    return VP_OK;
}

extern "C" {

int vp_distance_transform_u8(vp_ctx* ctx, const uint8_t* src, int w, int h, int metric, int dst_depth, void* dst)
{
    if (!src || !dst) return vp_fail(ctx, VP_ERR_INVALID, "vp_distance_transform_u8: a pointer is missing");
    const size_t es = dst_depth == VP_DEPTH_8U ? 1 : 4;
    if (const char* why = vp_distance_transform_refusal(w, h, w > 0 ? (size_t)w : 0, 1, 0, metric, dst_depth, w > 0 ? (size_t)w * es : 0))
        return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    const size_t npx = (size_t)w * h;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, npx);
    uint8_t* d_dst; W.want(&d_dst, npx * es);
    uint16_t* d_g; W.want(&d_g, vp_dist_g_bytes(w, h));
    VP_TRY(vp_ws_commit(ctx, W, "vp_distance_transform_u8"));
    VP_TRY(h2d(ctx, d_src, src, npx));
    VP_TRY(vpk_distance_transform(ctx, d_src, (size_t)w, w, h, nullptr, metric, dst_depth, d_g, d_dst, (size_t)w * es));
    VP_TRY(d2h(ctx, dst, d_dst, npx * es));
    return vp_synchronize(ctx);
}

int vp_distance_transform_dev(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, const unsigned long long* d_src_bits, int metric, int dst_depth,
                              void* d_dst, size_t dst_stride)
{
    if (const char* why = vp_distance_transform_refusal(w, h, stride, d_src != nullptr, d_src_bits != nullptr, metric, dst_depth, dst_stride))
        return vp_fail(ctx, VP_ERR_INVALID, why);
    if (!d_src || !d_dst) return vp_fail(ctx, VP_ERR_INVALID, "vp_distance_transform_dev: a pointer is missing");
    if (d_src_bits && (uintptr_t)d_src_bits % 8) return vp_fail(ctx, VP_ERR_INVALID, "vp_distance_transform_dev: the bit plane must be 8-byte aligned");
    const size_t es = dst_depth == VP_DEPTH_8U ? 1 : 4;
    if ((uintptr_t)d_dst % es || dev_overlap(d_src, strided_bytes(stride, (size_t)w, h), d_dst, strided_bytes(dst_stride, (size_t)w * es, h)))
        return vp_fail(ctx, VP_ERR_INVALID, "vp_distance_transform_dev: dst is not aligned to its element, or overlaps src");
    VP_TRY(check_ctx(ctx));
    vp_ws_frame W;
    uint16_t* d_g; W.want(&d_g, vp_dist_g_bytes(w, h));
    VP_TRY(vp_ws_commit(ctx, W, "vp_distance_transform_dev"));
    return vpk_distance_transform(ctx, d_src, stride, w, h, reinterpret_cast<const u64*>(d_src_bits), metric, dst_depth, d_g, d_dst, dst_stride);
}

int vp_min_max_loc_u8(vp_ctx* ctx, const void* src, size_t stride, int w, int h, int depth, const uint8_t* mask, size_t mask_stride, int mask_w, int mask_h,
                      void* out)
{
    if (!src || !out) return vp_fail(ctx, VP_ERR_INVALID, "vp_min_max_loc_u8: a pointer is missing");
    if (const char* why = vp_min_max_loc_refusal(w, h, stride, depth, mask != nullptr, mask_w, mask_h, mask_stride)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    const size_t npx = (size_t)w * h, es = depth == VP_DEPTH_8U ? 1 : 4, row = (size_t)w * es;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, npx * es);
    uint8_t* d_mask = nullptr;
    if (mask) W.want(&d_mask, npx);
    u64* d_keys; W.want(&d_keys, 16);
    VP_TRY(vp_ws_commit(ctx, W, "vp_min_max_loc_u8"));
    VP_TRY(h2d_rows(ctx, d_src, row, src, stride, row, h));
    if (mask) VP_TRY(h2d_rows(ctx, d_mask, (size_t)w, mask, mask_stride, (size_t)w, h));
    return min_max_loc_run(ctx, d_src, row, w, h, depth, d_mask, (size_t)w, nullptr, d_keys, (vp_min_max_loc_result*)out);
}

int vp_min_max_loc_dev(vp_ctx* ctx, const void* d_src, size_t stride, int w, int h, int depth, const uint8_t* d_mask, size_t mask_stride, int mask_w, int mask_h,
                       const unsigned long long* d_mask_bits, void* out)
{
    if (!d_src || !out) return vp_fail(ctx, VP_ERR_INVALID, "vp_min_max_loc_dev: a pointer is missing");
    if (d_mask_bits && (uintptr_t)d_mask_bits % 8) return vp_fail(ctx, VP_ERR_INVALID, "vp_min_max_loc_dev: the bit plane must be 8-byte aligned");
    const int has_mask = d_mask != nullptr || d_mask_bits != nullptr;
    if (const char* why = vp_min_max_loc_refusal(w, h, stride, depth, has_mask, mask_w, mask_h, d_mask ? mask_stride : (size_t)(w > 0 ? w : 0)))
        return vp_fail(ctx, VP_ERR_INVALID, why);
    if (depth == VP_DEPTH_32F && (uintptr_t)d_src % 4) return vp_fail(ctx, VP_ERR_INVALID, "vp_min_max_loc_dev: a float32 source must be 4-byte aligned");
    VP_TRY(check_ctx(ctx));
    vp_ws_frame W;
    u64* d_keys; W.want(&d_keys, 16);
    VP_TRY(vp_ws_commit(ctx, W, "vp_min_max_loc_dev"));
    return min_max_loc_run(ctx, d_src, stride, w, h, depth, d_mask_bits ? nullptr : d_mask, mask_stride, reinterpret_cast<const u64*>(d_mask_bits),
                           d_keys, (vp_min_max_loc_result*)out);
}

}  // extern "C"
