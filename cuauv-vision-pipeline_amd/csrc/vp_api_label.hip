// C ABI of libvp.so, labelling: connected components and contours of host images, device images and bit planes (kernels:
// vp_ccl + vp_contours.inl).
#include "vp_api_util.h"

extern "C" {

int vp_ccl_u8(vp_ctx* ctx, const uint8_t* src, size_t src_stride, int w, int h, int numbering, int32_t* labels, int32_t* stats,
              double* centroids, int max_labels, int32_t* nlabels)
{
    VP_TRY(check_ctx(ctx));
    if (!src || w <= 0 || h <= 0 || src_stride < (size_t)w || max_labels < 1 || !nlabels)
        return vp_fail(ctx, VP_ERR_INVALID, "vp_ccl_u8 arguments");
    if (numbering != VP_CCL_BLOCK2X2 && numbering != VP_CCL_PIXEL) return vp_fail(ctx, VP_ERR_INVALID, "numbering");
    const size_t npx = (size_t)w * h;
    const size_t bitbytes = (size_t)h * vp_ww(w) * 8;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, npx);
    u64* d_bits; W.want(&d_bits, bitbytes);
    int32_t* d_labels; W.want(&d_labels, npx * 4);
    int32_t* d_stats; W.want(&d_stats, (size_t)max_labels * 20);
    double* d_cent; W.want(&d_cent, (size_t)max_labels * 16);
    int32_t* d_nl; W.want(&d_nl, 4);
    vp_ccl_ws ws;
    vp_ccl_ws_want(W, w, h, 1, max_labels, &ws);
    VP_TRY(vp_ws_commit(ctx, W, "vp_ccl_u8"));
    VP_TRY(h2d_rows(ctx, d_src, (size_t)w, src, src_stride, (size_t)w, h));
    VP_TRY(vpk_pack_bits(ctx, d_src, (size_t)w, w, h, 1, d_bits, nullptr));
    VP_TRY(vpk_ccl(ctx, d_bits, w, h, 1, numbering, ws, labels ? d_labels : nullptr, d_stats, d_cent, max_labels, d_nl));
    VP_TRY(d2h(ctx, nlabels, d_nl, 4));
    if (labels) VP_TRY(d2h(ctx, labels, d_labels, npx * 4));
    if (stats) VP_TRY(d2h(ctx, stats, d_stats, (size_t)max_labels * 20));
    if (centroids) VP_TRY(d2h(ctx, centroids, d_cent, (size_t)max_labels * 16));
    return vp_synchronize(ctx);
}

// vp_ccl_u8 with the mask (or its bit plane) already in HBM; labels (nullable) stay there, the statistics come back
static int ccl_dev_impl(vp_ctx* ctx, const char* who, const uint8_t* d_src, size_t src_stride, const u64* bits_in, int w, int h, int numbering,
                        int32_t* d_labels, int32_t* stats, double* centroids, int max_labels, int32_t* nlabels)
{
    VP_TRY(check_ctx(ctx));
    if ((!d_src && !bits_in) || w <= 0 || h <= 0 || (!bits_in && src_stride < (size_t)w) || max_labels < 1 || !nlabels) return vp_fail(ctx, VP_ERR_INVALID, who);
    if (numbering != VP_CCL_BLOCK2X2 && numbering != VP_CCL_PIXEL) return vp_fail(ctx, VP_ERR_INVALID, "numbering");
    const size_t bitbytes = (size_t)h * vp_ww(w) * 8;
    vp_ws_frame W;
    u64* d_bits; W.want(&d_bits, bitbytes);
    int32_t* d_stats; W.want(&d_stats, (size_t)max_labels * 20);
    double* d_cent; W.want(&d_cent, (size_t)max_labels * 16);
    int32_t* d_nl; W.want(&d_nl, 4);
    vp_ccl_ws ws;
    vp_ccl_ws_want(W, w, h, 1, max_labels, &ws);
    VP_TRY(vp_ws_commit(ctx, W, "ccl_dev_impl"));
    const u64* bits = bits_in;
    if (!bits) {
        VP_TRY(vpk_pack_bits(ctx, d_src, src_stride, w, h, 1, d_bits, nullptr));
        bits = d_bits;
    }
    VP_TRY(vpk_ccl(ctx, bits, w, h, 1, numbering, ws, d_labels, d_stats, d_cent, max_labels, d_nl));
    VP_TRY(d2h(ctx, nlabels, d_nl, 4));
    if (stats) VP_TRY(d2h(ctx, stats, d_stats, (size_t)max_labels * 20));
    if (centroids) VP_TRY(d2h(ctx, centroids, d_cent, (size_t)max_labels * 16));
    return vp_synchronize(ctx);
}

int vp_ccl_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, int numbering, int32_t* d_labels, int32_t* stats, double* centroids,
               int max_labels, int32_t* nlabels)
{
    if (!d_src) return vp_fail(ctx, VP_ERR_INVALID, "vp_ccl_dev arguments");
    return ccl_dev_impl(ctx, "vp_ccl_dev arguments", d_src, src_stride, nullptr, w, h, numbering, d_labels, stats, centroids, max_labels, nlabels);
}

int vp_ccl_bits_dev(vp_ctx* ctx, const unsigned long long* d_bits, int w, int h, int numbering, int32_t* d_labels, int32_t* stats, double* centroids,
                    int max_labels, int32_t* nlabels)
{
    if (!d_bits) return vp_fail(ctx, VP_ERR_INVALID, "vp_ccl_bits_dev arguments");
    return ccl_dev_impl(ctx, "vp_ccl_bits_dev arguments", nullptr, 0, reinterpret_cast<const u64*>(d_bits), w, h, numbering, d_labels, stats, centroids,
                        max_labels, nlabels);
}

// src: host image (uploaded) or, with src_on_device, a device image read in place; or (bits_in) its bit-packed form, already on the device
static int find_contours_impl(vp_ctx* ctx, const uint8_t* src, bool src_on_device, size_t src_stride, int w, int h, int mode, int method,
                              int32_t* points, int64_t max_points, int32_t* counts, uint8_t* is_hole, int max_contours, int32_t* n_contours,
                              int64_t* n_points, const u64* bits_in = nullptr, int32_t* hierarchy = nullptr, bool tree_entry = false)
{
    VP_TRY(check_ctx(ctx));
    if ((!src && !bits_in) || w <= 0 || h <= 0 || (!bits_in && src_stride < (size_t)w) || !n_contours || !n_points || max_contours < 0 || max_points < 0)
        return vp_fail(ctx, VP_ERR_INVALID, "vp_find_contours arguments");
    const size_t npx = (size_t)w * h;
    const size_t bitbytes = (size_t)h * vp_ww(w) * 8;
    const int mc = max_contours > 0 ? max_contours : 1;
    const long long mp = max_points > 0 ? max_points : 1;
    // RETR_CCOMP / RETR_TREE (the tree entries only): the header carries the hierarchy rows [mc][4] between the offsets and the hole flags
    const bool tree = tree_entry && (mode == VP_RETR_CCOMP || mode == VP_RETR_TREE);
    const ct_hdr_layout L = ct_hdr(mc, tree);            // the result header, one block so that one copy brings it back (vp_contours_plan.h)
    const size_t hdr_bytes = L.bytes;
    vp_ws_frame W;
    uint8_t* d_stage; W.want(&d_stage, npx);
    u64* d_bits; W.want(&d_bits, bitbytes);
    uint8_t* d_hdr; W.want(&d_hdr, hdr_bytes);
    int32_t* d_points; W.want(&d_points, (size_t)mp * 8);
    const size_t ct_bytes = vp_contours_ws_bytes(w, h, 1, mc) + (tree ? vp_contour_tree_ws_bytes(mc) : 0);
    uint8_t* d_ct; W.want(&d_ct, ct_bytes);              // the pass's scratch: a repeated pass uses it again
    VP_TRY(vp_ws_commit(ctx, W, "find_contours_impl"));
    const uint8_t* d_src = d_stage;
    size_t d_stride = (size_t)w;
    // the header's arrays in the workspace block, or in the pinned one the kernels mirror them into
    auto hdr_at = [&](uint8_t* base) {
        vp_contour_mirror m = {};
        m.info = reinterpret_cast<int32_t*>(base);
        m.counts = reinterpret_cast<int32_t*>(base + L.counts);
        m.offsets = reinterpret_cast<int32_t*>(base + L.offsets);
        m.hier = tree ? reinterpret_cast<int32_t*>(base + L.hier) : nullptr;
        m.is_hole = base + L.is_hole;
        return m;
    };
    const vp_contour_mirror dh = hdr_at(d_hdr);
    const u64* bits_use = d_bits;
    if (bits_in) {
        bits_use = bits_in;                               // the caller made the bit plane with the mask (vp_inrange_u8_bits_dev): no packing launch
    } else {
        if (src_on_device) { d_src = src; d_stride = src_stride; }
        else VP_TRY(h2d_rows(ctx, d_stage, (size_t)w, src, src_stride, (size_t)w, h));
        VP_TRY(vpk_pack_bits(ctx, d_src, d_stride, w, h, 1, d_bits, nullptr));
    }
    // one block does the bookkeeping between the two follower passes - unless the last pass of this context met a speckled mask
    // (more border segments than the block's LDS tables hold): then it is launched over the chip (VP_CT_MANY=0 / 1: never / always)
    bool many_forced;
    const bool many = ct_want_many(ctx->ct.heads_hint, &many_forced);
    // The header and the first points come back without a copy: the kernels that make them write them into the pinned staging
    // buffer as well, and the call only synchronises (longer point lists take a copy afterwards).  VP_CT_MIRROR=0: a copy, as before.
    const size_t spec_pts = points ? (size_t)std::min<long long>(mp, 8192) : 0;
    const size_t hdr_pad = vp_align(hdr_bytes);
    uint8_t* hs = (uint8_t*)vp_hstage(ctx, hdr_pad + spec_pts * 8);
    if (!hs) return vp_fail(ctx, VP_ERR_NOMEM, "pinned staging");
    static const bool mirror_off = getenv("VP_CT_MIRROR") && atoi(getenv("VP_CT_MIRROR")) == 0;
    vp_contour_mirror hm = hdr_at(hs);
    hm.points = spec_pts ? reinterpret_cast<int32_t*>(hs + hdr_pad) : nullptr;
    hm.points_cap = (long long)spec_pts;
    // One block only up to what its LDS tables hold: a mask that turns out to have more heads than that while none was expected says so
    // in place of a result (0.1 ms), and the pass is repeated as launches - instead of one block working through 600 k heads in global
    // memory (9 ms at 10 % noise).  Not when a form is forced.
    bool many_now = many;
    const int32_t* info = nullptr;
    for (;;) {
        const bool defer = !many_now && !many_forced;
        VP_TRY(vpk_find_contours(ctx, d_ct, ct_bytes, bits_use, w, h, 1, mode, method, dh.counts, dh.is_hole, dh.offsets, d_points, mc, mp, dh.info, many_now,
                                 reinterpret_cast<uint32_t*>(dh.info + 2), mirror_off ? nullptr : &hm, defer, dh.hier));
        if (mirror_off) {
            if (spec_pts && reinterpret_cast<uint8_t*>(d_points) == d_hdr + hdr_pad) {
                VP_TRY(d2h(ctx, hs, d_hdr, hdr_pad + spec_pts * 8));           // header and points lie back to back in the workspace: one copy
            } else {
                VP_TRY(d2h(ctx, hs, d_hdr, hdr_bytes));
                if (spec_pts) VP_TRY(d2h(ctx, hs + hdr_pad, d_points, spec_pts * 8));
            }
        }
        VP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        info = reinterpret_cast<const int32_t*>(hs);
        ctx->ct.heads_hint = (uint32_t)info[2];
        if (info[0] != -1 || many_now) break;
        many_now = true;
    }
    if (info[0] < 0) return vp_fail(ctx, VP_ERR_HIP, "contours: no result");
    const int K = info[0];
    const int64_t P = info[1];
    *n_contours = K;
    *n_points = P;            // (the bookkeeping counts the points of every border, those beyond max_contours included)
    if (K > max_contours || P > max_points || K == 0) return VP_OK;
    std::vector<int32_t> hc(K), ho(K);
    std::vector<uint8_t> hh(K);
    memcpy(hc.data(), hs + L.counts, (size_t)K * 4);
    memcpy(ho.data(), hs + L.offsets, (size_t)K * 4);
    memcpy(hh.data(), hs + L.is_hole, (size_t)K);
    if (hierarchy) {
        // RETR_CCOMP / RETR_TREE: the rows came in cv2's order; the flat modes: each contour the next one's newer sibling
        if (tree) memcpy(hierarchy, hs + L.hier, (size_t)K * 16);
        else
            for (int j = 0; j < K; j++) {
                hierarchy[4 * j] = j + 1 < K ? j + 1 : -1;
                hierarchy[4 * j + 1] = j - 1;
                hierarchy[4 * j + 2] = -1;
                hierarchy[4 * j + 3] = -1;
            }
    }
    const int32_t* hp = reinterpret_cast<const int32_t*>(hs + hdr_pad);
    if (points && (size_t)P > spec_pts) {
        hs = (uint8_t*)vp_hstage(ctx, (size_t)P * 8 + 256);
        if (!hs) return vp_fail(ctx, VP_ERR_NOMEM, "pinned staging");
        VP_TRY(d2h(ctx, hs, d_points, (size_t)P * 8));
        VP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        hp = reinterpret_cast<const int32_t*>(hs);
    }
    // device order = discovery order; cv2 hands contours back newest first
    size_t o = 0;
    for (int k = K - 1, j = 0; k >= 0; k--, j++) {
        if (points) memcpy(points + 2 * o, hp + 2 * (size_t)ho[k], (size_t)hc[k] * 8);
        o += (size_t)hc[k];
        if (counts) counts[j] = hc[k];
        if (is_hole) is_hole[j] = hh[k];
    }
    return VP_OK;
}

int vp_find_contours_u8(vp_ctx* ctx, const uint8_t* src, size_t src_stride, int w, int h, int mode, int method, int32_t* points,
                        int64_t max_points, int32_t* counts, uint8_t* is_hole, int max_contours, int32_t* n_contours, int64_t* n_points)
{
    return find_contours_impl(ctx, src, false, src_stride, w, h, mode, method, points, max_points, counts, is_hole, max_contours, n_contours, n_points);
}

// the mask is a device image; the contour lists come back to host memory as with vp_find_contours_u8 (synchronised on return)
int vp_find_contours_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, int mode, int method, int32_t* points,
                         int64_t max_points, int32_t* counts, uint8_t* is_hole, int max_contours, int32_t* n_contours, int64_t* n_points)
{
    return find_contours_impl(ctx, d_src, true, src_stride, w, h, mode, method, points, max_points, counts, is_hole, max_contours, n_contours, n_points);
}

// the same with the hierarchy: modes VP_RETR_CCOMP / VP_RETR_TREE as well (vp.h)
int vp_find_contours_tree_u8(vp_ctx* ctx, const uint8_t* src, size_t src_stride, int w, int h, int mode, int method, int32_t* points,
                             int64_t max_points, int32_t* counts, uint8_t* is_hole, int max_contours, int32_t* n_contours, int64_t* n_points,
                             int32_t* hierarchy)
{
    return find_contours_impl(ctx, src, false, src_stride, w, h, mode, method, points, max_points, counts, is_hole, max_contours, n_contours, n_points,
                              nullptr, hierarchy, true);
}

int vp_find_contours_tree_dev(vp_ctx* ctx, const uint8_t* d_src, size_t src_stride, int w, int h, int mode, int method, int32_t* points,
                              int64_t max_points, int32_t* counts, uint8_t* is_hole, int max_contours, int32_t* n_contours, int64_t* n_points,
                              int32_t* hierarchy)
{
    return find_contours_impl(ctx, d_src, true, src_stride, w, h, mode, method, points, max_points, counts, is_hole, max_contours, n_contours, n_points,
                              nullptr, hierarchy, true);
}

int vp_find_contours_tree_bits_dev(vp_ctx* ctx, const unsigned long long* d_bits, int w, int h, int mode, int method, int32_t* points,
                                   int64_t max_points, int32_t* counts, uint8_t* is_hole, int max_contours, int32_t* n_contours, int64_t* n_points,
                                   int32_t* hierarchy)
{
    return find_contours_impl(ctx, nullptr, true, 0, w, h, mode, method, points, max_points, counts, is_hole, max_contours, n_contours, n_points,
                              reinterpret_cast<const u64*>(d_bits), hierarchy, true);
}

unsigned int vp_contours_last_heads(vp_ctx* ctx)
{
    if (!ctx) return 0;
    const uint32_t b = vp_ct_batch_hint(ctx);
    return b > ctx->ct.heads_hint ? b : ctx->ct.heads_hint;
}

int vp_find_contours_bits_dev(vp_ctx* ctx, const unsigned long long* d_bits, int w, int h, int mode, int method, int32_t* points, int64_t max_points,
                              int32_t* counts, uint8_t* is_hole, int max_contours, int32_t* n_contours, int64_t* n_points)
{
    return find_contours_impl(ctx, nullptr, true, 0, w, h, mode, method, points, max_points, counts, is_hole, max_contours, n_contours, n_points,
                              reinterpret_cast<const u64*>(d_bits));
}

}  // extern "C"
