// C ABI of libvp.so, colour k-means: the clustering of a uint8 image's pixels on host and device images, and the masks of a label
// image (kernels: vp_kmeans.hip; checks, geometry, the device table's layout and the compactness: vp_kmeans_plan.h).
#include "vp_api_util.h"
#include "vp_kmeans_plan.h"

// The whole loop on the device, the optional copy of the labels to labels_host (packed), the table back through pinned staging and one
// synchronise; b is in the caller's frame (kmeans_want).  lstride in bytes.
struct kmeans_bufs { uint8_t *table, *init; };
static void kmeans_want(vp_ws_frame& W, int k, int cn, kmeans_bufs* b)
{
    W.want(&b->table, vp_kmeans_table_bytes(k, cn));
    W.want(&b->init, (size_t)k * cn * 4);
}
static int kmeans_run(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int cn, int k, const float* centers_init, const int32_t* seed_index,
                      int max_iter, double eps, int32_t* d_labels, size_t lstride, int32_t* labels_host, void* out, const kmeans_bufs& b)
{
    const size_t tbytes = vp_kmeans_table_bytes(k, cn);
    uint8_t *d_table = b.table, *d_init = b.init;
    if (centers_init) VP_TRY(h2d(ctx, d_init, centers_init, (size_t)k * cn * 4));
    else VP_TRY(h2d(ctx, d_init, seed_index, (size_t)k * 4));
    VP_TRY(vpk_kmeans(ctx, d_src, stride, w, h, cn, k, centers_init ? (const float*)d_init : nullptr, centers_init ? nullptr : (const int32_t*)d_init, max_iter, eps,
                      d_table, d_labels, lstride / 4));
    if (labels_host) VP_TRY(d2h(ctx, labels_host, d_labels, (size_t)w * h * 4));
    uint8_t* ht = (uint8_t*)vp_hstage(ctx, tbytes);
    if (!ht) return vp_fail(ctx, VP_ERR_NOMEM, "pinned staging");
    VP_TRY(d2h(ctx, ht, d_table, tbytes));
    VP_TRY(vp_synchronize(ctx));
    const uint32_t* state = (const uint32_t*)(ht + vp_kmeans_off_state(k, cn));
    const float* centres = (const float*)(ht + vp_kmeans_off_centres(k, cn));
    const uint32_t* n = (const uint32_t*)(ht + vp_kmeans_off_n(k, cn));
    vp_kmeans_result_head head;
    head.compactness = vp_kmeans_compactness(k, cn, centres, n, (const uint32_t*)(ht + vp_kmeans_off_s1(k, cn)), (const uint64_t*)(ht + vp_kmeans_off_s2(k, cn)));
    head.iterations = (int32_t)state[1];
    head.k = k;
    uint8_t* o = (uint8_t*)out;
    memcpy(o, &head, sizeof head);
    memcpy(o + sizeof head, centres, (size_t)k * cn * 4);
    memcpy(o + sizeof head + (size_t)k * cn * 4, n, (size_t)k * 4);
    return VP_OK;
}

extern "C" {

int vp_kmeans_u8(vp_ctx* ctx, const uint8_t* src, int w, int h, int cn, int k, const float* centers_init, const int32_t* seed_index, int max_iter, double eps,
                 int32_t* labels, void* out)
{
    if (!src || !out) return vp_fail(ctx, VP_ERR_INVALID, "vp_kmeans_u8: a pointer is missing");
    if (const char* why = vp_kmeans_refusal(w, h, w > 0 && cn > 0 ? (size_t)w * cn : 0, cn, k, centers_init, seed_index, max_iter, eps))
        return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    const size_t npx = (size_t)w * h;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, npx * cn);
    int32_t* d_labels = nullptr;
    if (labels) W.want(&d_labels, npx * 4);
    kmeans_bufs b;
    kmeans_want(W, k, cn, &b);
    VP_TRY(vp_ws_commit(ctx, W, "vp_kmeans_u8"));
    VP_TRY(h2d(ctx, d_src, src, npx * cn));
    return kmeans_run(ctx, d_src, (size_t)w * cn, w, h, cn, k, centers_init, seed_index, max_iter, eps, d_labels, (size_t)w * 4, labels, out, b);
}

int vp_kmeans_dev(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int cn, int k, const float* centers_init, const int32_t* seed_index,
                  int max_iter, double eps, int32_t* d_labels, size_t labels_stride, void* out)
{
    if (!d_src || !out) return vp_fail(ctx, VP_ERR_INVALID, "vp_kmeans_dev: a pointer is missing");
    if (const char* why = vp_kmeans_refusal(w, h, stride, cn, k, centers_init, seed_index, max_iter, eps)) return vp_fail(ctx, VP_ERR_INVALID, why);
    if (d_labels) {
        if (const char* why = vp_kmeans_labels_refusal(w, labels_stride)) return vp_fail(ctx, VP_ERR_INVALID, why);
        if ((uintptr_t)d_labels % 4 || dev_overlap(d_src, strided_bytes(stride, (size_t)w * cn, h), d_labels, strided_bytes(labels_stride, (size_t)w * 4, h)))
            return vp_fail(ctx, VP_ERR_INVALID, "vp_kmeans_dev: the labels are not 4-byte aligned, or overlap the source");
    }
    VP_TRY(check_ctx(ctx));
    vp_ws_frame W;
    kmeans_bufs b;
    kmeans_want(W, k, cn, &b);
    VP_TRY(vp_ws_commit(ctx, W, "vp_kmeans_dev"));
    return kmeans_run(ctx, d_src, stride, w, h, cn, k, centers_init, seed_index, max_iter, eps, d_labels, labels_stride, nullptr, out, b);
}

int vp_label_select_dev(vp_ctx* ctx, const int32_t* d_labels, size_t labels_stride, int w, int h, const uint8_t* select, int k, uint8_t* d_mask,
                        size_t mask_stride, unsigned long long* d_mask_bits)
{
    if (!d_labels || !select || !d_mask) return vp_fail(ctx, VP_ERR_INVALID, "vp_label_select_dev: a pointer is missing");
    if (const char* why = vp_label_select_refusal(w, h, labels_stride, k, mask_stride)) return vp_fail(ctx, VP_ERR_INVALID, why);
    if ((uintptr_t)d_labels % 4) return vp_fail(ctx, VP_ERR_INVALID, "vp_label_select_dev: the labels must be 4-byte aligned");
    if (d_mask_bits && (uintptr_t)d_mask_bits % 8) return vp_fail(ctx, VP_ERR_INVALID, "vp_label_select_dev: the bit plane must be 8-byte aligned");
    if (dev_overlap(d_labels, strided_bytes(labels_stride, (size_t)w * 4, h), d_mask, strided_bytes(mask_stride, (size_t)w, h)))
        return vp_fail(ctx, VP_ERR_INVALID, "vp_label_select_dev: the mask overlaps the labels");
    VP_TRY(check_ctx(ctx));
    return vpk_label_select(ctx, d_labels, labels_stride / 4, w, h, select, k, d_mask, mask_stride, reinterpret_cast<u64*>(d_mask_bits));
}

}  // extern "C"
