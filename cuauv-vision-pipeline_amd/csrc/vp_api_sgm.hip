// C ABI of libvp.so, semi-global stereo matching: disparity of a rectified pair with a left-right check, on host and device images
// (kernels: vp_sgm.hip; checks, geometry and workspace: vp_sgm_plan.h), and the same statement as plain scalar C++.
#include "vp_api_util.h"
#include "vp_sgm_plan.h"

int vpk_stereo_sgm(vp_ctx* ctx, const uint8_t* d_left, size_t lstride, const uint8_t* d_right, size_t rstride, int w, int h, int nd, int min_disp, int cap, int p1, int p2,
                   int uniq, int diff, int paths, const vp_sgm_plan& P, uint8_t* d_ws, int16_t* d_disp, size_t dstride);

// everything the three matcher entries refuse, from the arguments alone
static const char* sgm_check(const uint8_t* left, size_t lstride, const uint8_t* right, size_t rstride, int w, int h, int nd, int block, int min_disp, int cap, int p1, int p2,
                             int uniq, int diff, int paths, const int16_t* disp, size_t dstride)
{
    if (!left || !right || !disp) return "sgm: a pointer is missing";
    if (const char* why = vp_sgm_refusal(w, h, lstride, rstride, nd, block, min_disp, cap, p1, p2, uniq, diff, paths, dstride)) return why;
    if ((uintptr_t)disp % 2) return "sgm: the result is not aligned to its element size";
    const size_t dbytes = strided_bytes(dstride, (size_t)w * 2, h);
    if (dev_overlap(left, strided_bytes(lstride, w, h), disp, dbytes) || dev_overlap(right, strided_bytes(rstride, w, h), disp, dbytes))
        return "sgm: the result overlaps an input image";
    return nullptr;
}

extern "C" {

int vp_stereo_sgm_plan(int w, int h, int num_disparities, int block_size, int min_disparity, int paths, int32_t* rect, size_t* ws_bytes, int32_t* geometry)
{
    if (!rect || !ws_bytes || !geometry) return vp_fail(nullptr, VP_ERR_INVALID, "vp_stereo_sgm_plan: a pointer is missing");
    if (const char* why = vp_sgm_geometry_refusal(w, h, num_disparities, block_size, min_disparity, paths)) return vp_fail(nullptr, VP_ERR_INVALID, why);
    vp_sgm_plan P;
    vp_sgm_make_plan(w, h, num_disparities, block_size, min_disparity, paths, &P);
    rect[0] = P.cw ? P.cx0 : 0;
    rect[1] = P.cw ? P.cy0 : 0;
    rect[2] = P.cw;
    rect[3] = P.ch;
    *ws_bytes = P.ws_bytes;
    const int32_t g[VP_SGM_GEOMETRY] = {SG_COST_THREADS, SG_STRIP, (int32_t)P.cost_gx, (int32_t)P.cost_gy, (int32_t)P.cost_lds,
                                        SG_AGG_THREADS, P.group, P.per_lane, P.lines_per_block, (int32_t)P.agg_gh, (int32_t)P.agg_gv, (int32_t)P.agg_gd,
                                        SG_SEL_THREADS, P.px_per_block, (int32_t)P.sel_g};
    memcpy(geometry, g, sizeof g);
    return VP_OK;
}

int vp_stereo_sgm_dev(vp_ctx* ctx, const uint8_t* left_dev, size_t left_stride, const uint8_t* right_dev, size_t right_stride, int w, int h, int num_disparities,
                      int block_size, int min_disparity, int pre_filter_cap, int p1, int p2, int uniqueness_ratio, int disp12_max_diff, int paths, int16_t* disp_dev,
                      size_t disp_stride)
{
    if (const char* why = sgm_check(left_dev, left_stride, right_dev, right_stride, w, h, num_disparities, block_size, min_disparity, pre_filter_cap, p1, p2, uniqueness_ratio,
                                    disp12_max_diff, paths, disp_dev, disp_stride))
        return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    vp_sgm_plan P;
    vp_sgm_make_plan(w, h, num_disparities, block_size, min_disparity, paths, &P);
    vp_ws_frame W;
    uint8_t* d_ws; W.want(&d_ws, P.ws_bytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_stereo_sgm_dev"));
    return vpk_stereo_sgm(ctx, left_dev, left_stride, right_dev, right_stride, w, h, num_disparities, min_disparity, pre_filter_cap, p1, p2, uniqueness_ratio, disp12_max_diff,
                          paths, P, d_ws, disp_dev, disp_stride);
}

int vp_stereo_sgm_u8(vp_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, int num_disparities, int block_size, int min_disparity, int pre_filter_cap, int p1,
                     int p2, int uniqueness_ratio, int disp12_max_diff, int paths, int16_t* disp)
{
    const size_t row = w > 0 ? (size_t)w : 0;
    if (const char* why = sgm_check(left, row, right, row, w, h, num_disparities, block_size, min_disparity, pre_filter_cap, p1, p2, uniqueness_ratio, disp12_max_diff, paths,
                                    disp, row * 2))
        return vp_fail(ctx, VP_ERR_INVALID, why);
    VP_TRY(check_ctx(ctx));
    vp_sgm_plan P;
    vp_sgm_make_plan(w, h, num_disparities, block_size, min_disparity, paths, &P);
    vp_ws_frame W;
    uint8_t* d_left; W.want(&d_left, row * h);
    uint8_t* d_right; W.want(&d_right, row * h);
    int16_t* d_disp; W.want(&d_disp, row * 2 * h);
    uint8_t* d_ws; W.want(&d_ws, P.ws_bytes);
    VP_TRY(vp_ws_commit(ctx, W, "vp_stereo_sgm_u8"));
    VP_TRY(h2d(ctx, d_left, left, row * h));
    VP_TRY(h2d(ctx, d_right, right, row * h));
    VP_TRY(vpk_stereo_sgm(ctx, d_left, row, d_right, row, w, h, num_disparities, min_disparity, pre_filter_cap, p1, p2, uniqueness_ratio, disp12_max_diff, paths, P, d_ws,
                          d_disp, row * 2));
    VP_TRY(d2h(ctx, disp, d_disp, row * 2 * h));
    return vp_synchronize(ctx);
}

int vp_stereo_sgm_host(const uint8_t* left, size_t left_stride, const uint8_t* right, size_t right_stride, int w, int h, int num_disparities, int block_size,
                       int min_disparity, int pre_filter_cap, int p1, int p2, int uniqueness_ratio, int disp12_max_diff, int paths, int16_t* disp, size_t disp_stride)
{
    if (const char* why = sgm_check(left, left_stride, right, right_stride, w, h, num_disparities, block_size, min_disparity, pre_filter_cap, p1, p2, uniqueness_ratio,
                                    disp12_max_diff, paths, disp, disp_stride))
        return vp_fail(nullptr, VP_ERR_INVALID, why);
    vp_sgm_plan P;
    vp_sgm_make_plan(w, h, num_disparities, block_size, min_disparity, paths, &P);
    const int nd = num_disparities, r = P.r, cw = P.cw, ch = P.ch, inv = vp_stereo_invalid(min_disparity);
    const size_t dpitch = disp_stride / 2;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) disp[(size_t)y * dpitch + x] = (int16_t)inv;
    if (!cw) return VP_OK;
    std::vector<uint8_t> pl((size_t)w * h), pr((size_t)w * h);
    vp_stereo_host_prefilter(left, left_stride, w, h, pre_filter_cap, pl.data());
    vp_stereo_host_prefilter(right, right_stride, w, h, pre_filter_cap, pr.data());

    // C[y][x][d]: per row, the sums over the window's rows per column of [vx0, vx0 + vn), then a running sum over 2 r + 1 columns
    const size_t vol = (size_t)cw * ch * nd;
    std::vector<uint16_t> C(vol), S(vol, 0);
    const int vx0 = P.cx0 - r, vn = cw + 2 * r;
    std::vector<int32_t> V(vn);
    for (int y = 0; y < ch; y++)
        for (int d = 0; d < nd; d++) {
            const int D = min_disparity + d;
            for (int i = 0; i < vn; i++) {
                int32_t v = 0;
                for (int j = -r; j <= r; j++) {
                    const size_t row = (size_t)(P.cy0 + y + j) * w;
                    v += std::abs((int)pl[row + vx0 + i] - (int)pr[row + vx0 + i - D]);
                }
                V[i] = v;
            }
            int32_t acc = 0;
            for (int k = 0; k <= 2 * r; k++) acc += V[k];
            for (int x = 0;; x++) {
                C[((size_t)y * cw + x) * nd + d] = (uint16_t)acc;
                if (x + 1 == cw) break;
                acc += V[x + 2 * r + 1] - V[x];
            }
        }

    // one direction at a time in the raster order in which a pixel's predecessor comes first; only two rows of L are kept
    std::vector<int32_t> Lrow[2] = {std::vector<int32_t>((size_t)cw * nd), std::vector<int32_t>((size_t)cw * nd)};
    std::vector<int32_t> Mrow[2] = {std::vector<int32_t>(cw), std::vector<int32_t>(cw)};
    for (int i = 0; i < paths; i++) {
        const int dy = vp_sgm_dirs[i][0], dx = vp_sgm_dirs[i][1];
        for (int yi = 0; yi < ch; yi++) {
            const int y = dy >= 0 ? yi : ch - 1 - yi, cur = yi & 1, prev = dy == 0 ? cur : cur ^ 1;
            for (int xi = 0; xi < cw; xi++) {
                const int x = dx >= 0 ? xi : cw - 1 - xi, qx = x - dx, qy = y - dy;
                const bool has_q = qx >= 0 && qx < cw && qy >= 0 && qy < ch;
                const uint16_t* c = C.data() + ((size_t)y * cw + x) * nd;
                uint16_t* s = S.data() + ((size_t)y * cw + x) * nd;
                int32_t* L = Lrow[cur].data() + (size_t)x * nd;
                int32_t m = INT32_MAX;
                if (!has_q) {
                    for (int d = 0; d < nd; d++) { L[d] = c[d]; m = std::min(m, L[d]); }
                } else {
                    const int32_t* Q = Lrow[prev].data() + (size_t)qx * nd;
                    const int32_t Mq = Mrow[prev][qx];
                    // with dy == 0 the predecessor shares the row buffer but not the pixel: Q and L never alias
                    for (int d = 0; d < nd; d++) {
                        int32_t best = std::min(Q[d], Mq + p2);
                        if (d > 0) best = std::min(best, Q[d - 1] + p1);
                        if (d < nd - 1) best = std::min(best, Q[d + 1] + p1);
                        L[d] = c[d] + best - Mq;
                        m = std::min(m, L[d]);
                    }
                }
                Mrow[cur][x] = m;
                for (int d = 0; d < nd; d++) s[d] = (uint16_t)(s[d] + L[d]);
            }
        }
    }

    for (int y = 0; y < ch; y++)
        for (int x = 0; x < cw; x++) {
            const uint16_t* s = S.data() + ((size_t)y * cw + x) * nd;
            int ds = 0, smin = s[0];
            for (int d = 1; d < nd; d++)
                if (s[d] <= smin) { smin = s[d]; ds = d; }
            if (uniqueness_ratio > 0) {
                const int limit = smin + smin * uniqueness_ratio / 100;
                bool rival = false;
                for (int d = 0; d < nd && !rival; d++) rival = (d < ds - 1 || d > ds + 1) && s[d] <= limit;
                if (rival) continue;
            }
            if (disp12_max_diff >= 0) {
                int dr = -1, best = INT32_MAX;
                for (int d = 0; d < nd; d++) {
                    const int xc = x - ds + d;
                    if (xc < 0 || xc >= cw) continue;
                    const int v = S[((size_t)y * cw + xc) * nd + d];
                    if (v <= best) { best = v; dr = d; }
                }
                if (std::abs(dr - ds) > disp12_max_diff) continue;
            }
            const int dm = ds > 0 ? ds - 1 : ds + 1, dq = ds < nd - 1 ? ds + 1 : ds - 1;
            disp[(size_t)(P.cy0 + y) * dpitch + P.cx0 + x] = vp_stereo_subpixel(smin, s[dm], s[dq], min_disparity + ds);
        }
    return VP_OK;
}

}  // extern "C"
