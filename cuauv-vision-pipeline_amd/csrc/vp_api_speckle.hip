// C ABI of libvp.so, what follows stereo matching: the speckle filter of an int16 disparity image and the surface normals of a depth
// image, on host and device images (kernels: vp_speckle.hip; checks, geometry and the normal's formula: vp_speckle_plan.h), and the
// same statements as plain scalar C++.
#include "vp_api_util.h"
#include "vp_speckle_plan.h"

int vpk_filter_speckles(vp_ctx* ctx, const int16_t* d_src, size_t sstride, int w, int h, int new_val, int max_size, int max_diff, const vp_speckle_plan& P, uint8_t* d_ws,
                        int16_t* d_dst, size_t dstride);
int vpk_normals(vp_ctx* ctx, const float* d_depth, size_t zstride, int w, int h, double f, double cx, double cy, double jump, int encode, float* d_normals, size_t nstride);

// everything the three filter entries refuse, from the arguments alone
static const char* speckle_check(const int16_t* src, size_t sstride, int w, int h, int new_val, int max_size, int max_diff, const int16_t* dst, size_t dstride)
{
    if (!src || !dst) return "filter_speckles: a pointer is missing";
    if (const char* why = vp_speckle_refusal(w, h, sstride, dstride, new_val, max_size, max_diff)) return why;
    if ((uintptr_t)src % 2 || (uintptr_t)dst % 2) return "filter_speckles: an image is not aligned to its element size";
    // cv2 filters in place: the very same image is admitted, any other shared byte is not
    if (!(dst == src && dstride == sstride) && dev_overlap(src, strided_bytes(sstride, (size_t)w * 2, h), dst, strided_bytes(dstride, (size_t)w * 2, h)))
        return "filter_speckles: the result overlaps the input without being the input (dst == src with one stride is allowed)";
    return nullptr;
}

static const char* normals_check(const float* depth, size_t zstride, int w, int h, double focal_px, double cx, double cy, double max_jump_m, const float* normals,
                                 size_t nstride)
{
    if (!depth || !normals) return "normals: a pointer is missing";
    if (const char* why = vp_normals_refusal(w, h, zstride, nstride, focal_px, cx, cy, max_jump_m)) return why;
    if ((uintptr_t)depth % 4 || (uintptr_t)normals % 4) return "normals: an image is not aligned to its element size";
    if (dev_overlap(depth, strided_bytes(zstride, (size_t)w * 4, h), normals, strided_bytes(nstride, (size_t)w * 12, h))) return "normals: the result overlaps the depth";
    return nullptr;
}

extern "C" {

int vp_filter_speckles_plan(int w, int h, size_t* ws_bytes, int32_t* geometry)
{
    if (!ws_bytes || !geometry) return vp_fail(nullptr, VP_ERR_INVALID, "vp_filter_speckles_plan: a pointer is missing");
    if (const char* why = vp_speckle_geometry_refusal(w, h)) return vp_fail(nullptr, VP_ERR_INVALID, why);
    vp_speckle_plan P;
    vp_speckle_make_plan(w, h, &P);
    *ws_bytes = P.ws_bytes;
    geometry[0] = P.tile;
    geometry[1] = P.tile;
    geometry[2] = (int32_t)P.grid_x;
    geometry[3] = (int32_t)P.grid_y;
    geometry[4] = (int32_t)P.lds_bytes;
    return VP_OK;
}

int vp_filter_speckles_dev(vp_ctx* ctx, const int16_t* src_dev, size_t src_stride, int w, int h, int new_val, int max_speckle_size, int max_diff, int16_t* dst_dev,
                           size_t dst_stride)
{
    if (const char* why = speckle_check(src_dev, src_stride, w, h, new_val, max_speckle_size, max_diff, dst_dev, dst_stride)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    vp_speckle_plan P;
    vp_speckle_make_plan(w, h, &P);
    vp_ws_frame W;
    uint8_t* d_ws; W.want(&d_ws, P.ws_bytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_filter_speckles_dev"));
    return vpk_filter_speckles(ctx, src_dev, src_stride, w, h, new_val, max_speckle_size, max_diff, P, d_ws, dst_dev, dst_stride);
}

int vp_filter_speckles_i16(vp_ctx* ctx, const int16_t* src, int w, int h, int new_val, int max_speckle_size, int max_diff, int16_t* dst)
{
    const size_t row = w > 0 ? (size_t)w * 2 : 0;
    if (const char* why = speckle_check(src, row, w, h, new_val, max_speckle_size, max_diff, dst, row)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    vp_speckle_plan P;
    vp_speckle_make_plan(w, h, &P);
    vp_ws_frame W;
    int16_t* d_img; W.want(&d_img, row * h);
    uint8_t* d_ws; W.want(&d_ws, P.ws_bytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_filter_speckles_i16"));
    VP_TRY(h2d(ctx, d_img, src, row * h));
    VP_TRY(vpk_filter_speckles(ctx, d_img, row, w, h, new_val, max_speckle_size, max_diff, P, d_ws, d_img, row));
    VP_TRY(d2h(ctx, dst, d_img, row * h));
    return vp_synchronize(ctx);
}

int vp_filter_speckles_host(const int16_t* src, size_t src_stride, int w, int h, int new_val, int max_speckle_size, int max_diff, int16_t* dst, size_t dst_stride)
{
    if (const char* why = speckle_check(src, src_stride, w, h, new_val, max_speckle_size, max_diff, dst, dst_stride)) return vp_fail(nullptr, VP_ERR_INVALID, why);
    const size_t sp = src_stride / 2, dp = dst_stride / 2, n = (size_t)w * h;
    std::vector<uint8_t> state(n, 0);        // 0 not visited, 1 kept, 2 removed
    std::vector<int32_t> region;             // the pixels of the region being filled, in the order found: a queue and the record in one
    region.reserve(n);
    for (int sy = 0; sy < h; sy++)
        for (int sx = 0; sx < w; sx++) {
            const size_t seed = (size_t)sy * w + sx;
            if (state[seed] || src[(size_t)sy * sp + sx] == new_val) continue;
            region.clear();
            region.push_back((int32_t)seed);
            state[seed] = 1;
            for (size_t at = 0; at < region.size(); at++) {
                const int x = region[at] % w, y = region[at] / w, v = src[(size_t)y * sp + x];
                const int nx[4] = {x - 1, x + 1, x, x}, ny[4] = {y, y, y - 1, y + 1};
                for (int k = 0; k < 4; k++) {
                    if (nx[k] < 0 || nx[k] >= w || ny[k] < 0 || ny[k] >= h) continue;
                    const size_t q = (size_t)ny[k] * w + nx[k];
                    const int u = src[(size_t)ny[k] * sp + nx[k]];
                    if (state[q] || u == new_val || !vp_speckle_linked(u, v, max_diff)) continue;
                    state[q] = 1;
                    region.push_back((int32_t)q);
                }
            }
            if (region.size() <= (size_t)max_speckle_size)
                for (int32_t p : region) state[p] = 2;
        }
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) dst[(size_t)y * dp + x] = state[(size_t)y * w + x] == 2 ? (int16_t)new_val : src[(size_t)y * sp + x];
    return VP_OK;
}

int vp_normals_from_depth_dev(vp_ctx* ctx, const float* depth_dev, size_t depth_stride, int w, int h, double focal_px, double cx, double cy, double max_jump_m, int encode,
                              float* normals_dev, size_t normals_stride)
{
    if (const char* why = normals_check(depth_dev, depth_stride, w, h, focal_px, cx, cy, max_jump_m, normals_dev, normals_stride)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    return vpk_normals(ctx, depth_dev, depth_stride, w, h, focal_px, cx, cy, vp_normals_jump(max_jump_m), encode != 0, normals_dev, normals_stride);
}

int vp_normals_from_depth_f32(vp_ctx* ctx, const float* depth, int w, int h, double focal_px, double cx, double cy, double max_jump_m, int encode, float* normals)
{
    const size_t n = w > 0 ? (size_t)w : 0;
    if (const char* why = normals_check(depth, n * 4, w, h, focal_px, cx, cy, max_jump_m, normals, n * 12)) return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    vp_ws_frame W;
    float* d_depth; W.want(&d_depth, n * 4 * h);
    float* d_normals; W.want(&d_normals, n * 12 * h);
    VP_TRY(vp_ws_commit(ctx, W, "vp_normals_from_depth_f32"));
    VP_TRY(h2d(ctx, d_depth, depth, n * 4 * h));
    VP_TRY(vpk_normals(ctx, d_depth, n * 4, w, h, focal_px, cx, cy, vp_normals_jump(max_jump_m), encode != 0, d_normals, n * 12));
    VP_TRY(d2h(ctx, normals, d_normals, n * 12 * h));
    return vp_synchronize(ctx);
}

int vp_normals_from_depth_host(const float* depth, size_t depth_stride, int w, int h, double focal_px, double cx, double cy, double max_jump_m, int encode, float* normals,
                               size_t normals_stride)
{
    if (const char* why = normals_check(depth, depth_stride, w, h, focal_px, cx, cy, max_jump_m, normals, normals_stride)) return vp_fail(nullptr, VP_ERR_INVALID, why);
    const double jump = vp_normals_jump(max_jump_m);
    const size_t zp = depth_stride / 4, np = normals_stride / 4;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            float n[3] = {0.0f, 0.0f, 0.0f};
            bool have = false;
            if (x >= 1 && y >= 1 && x <= w - 2 && y <= h - 2) {
                const float* z = depth + (size_t)y * zp + x;
                have = vp_normal_at(x, y, z[0], z[-1], z[1], z[-(ptrdiff_t)zp], z[zp], focal_px, cx, cy, jump, n);
            }
            vp_normal_store(have, n, encode != 0, normals + (size_t)y * np + (size_t)x * 3);
        }
    return VP_OK;
}

}  // extern "C"
