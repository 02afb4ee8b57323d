// C ABI of libvp.so, contour geometry: the three forms of the device pass (kernel: vp_geometry), the host functions that finish its raw
// rows, and the host-only enclosing circle.  Every size rule and refusal is vp_geometry_plan.h's.
#include "vp_api_util.h"
#include "vp_geometry_plan.h"

static_assert(sizeof(vp_geom_raw) == 64, "the raw row is 64 bytes");
static_assert(sizeof(vp_contour_geom) == 80, "vp_contour_geom is 80 bytes (vision/_vp.py mirrors it)");
static_assert((int)GEOM_ST_HULL_CAP == VP_GEOM_HULL_CAP && (int)GEOM_ST_PERIMETER == VP_GEOM_PERIMETER && (int)GEOM_ST_SKIPPED == VP_GEOM_SKIPPED &&
              (int)GEOM_ST_COORD == VP_GEOM_COORD, "status bits of the plan and of vp.h");

// centre and radius from an exact support set: x0 + Dx / (2 D) with integer Dx, D (below 2^53), one division and one addition per
// coordinate; the radius is the double root of the squared distance to the first support point; each rounded to float once
static void circle_from_support(const vp_geom_support& s, float* out3)
{
    out3[0] = out3[1] = out3[2] = 0.f;
    if (s.n <= 0) return;
    if (s.n == 1) { out3[0] = (float)s.x[0]; out3[1] = (float)s.y[0]; return; }
    double ux, uy;
    if (s.n == 2) {
        ux = (double)(s.x[1] - s.x[0]) / 2.0;
        uy = (double)(s.y[1] - s.y[0]) / 2.0;
    } else {
        const long long bx = s.x[1] - s.x[0], by = s.y[1] - s.y[0], cx = s.x[2] - s.x[0], cy = s.y[2] - s.y[0];
        const long long b2 = bx * bx + by * by, c2 = cx * cx + cy * cy;
        const long long d2 = 2 * (bx * cy - by * cx);
        const long long dx = cy * b2 - by * c2, dy = bx * c2 - cx * b2;
        ux = (double)dx / (double)d2;
        uy = (double)dy / (double)d2;
    }
    out3[0] = (float)((double)s.x[0] + ux);
    out3[1] = (float)((double)s.y[0] + uy);
    out3[2] = (float)sqrt(ux * ux + uy * uy);
}

// the incremental algorithm of the kernel, one vertex at a time, in the kernel's order: the same support set
static void support_of_hull(const int32_t* hull, int h, vp_geom_support* C)
{
    C->n = 0;
    for (int k = 0; k < 3; k++) C->x[k] = C->y[k] = 0;
    if (h <= 0) return;
    const int stride = vp_geom_stride(h);
    auto vx = [&](int t) { return hull + 2 * (int)(((long long)t * stride) % h); };
    C->n = 1; C->x[0] = vx(0)[0]; C->y[0] = vx(0)[1];
    for (int i = 1; i < h; i++) {
        if (!vp_geom_outside(*C, vx(i)[0], vx(i)[1])) continue;
        C->n = 1; C->x[0] = vx(i)[0]; C->y[0] = vx(i)[1];
        for (int j = 0; j < i; j++) {
            if (!vp_geom_outside(*C, vx(j)[0], vx(j)[1])) continue;
            C->n = 2; C->x[1] = vx(j)[0]; C->y[1] = vx(j)[1];
            for (int k = 0; k < j; k++) {
                if (!vp_geom_outside(*C, vx(k)[0], vx(k)[1])) continue;
                C->n = 3; C->x[2] = vx(k)[0]; C->y[2] = vx(k)[1];
            }
        }
    }
}

static void store_support(const vp_geom_support& s, vp_contour_geom* g)
{
    g->support_count = s.n;
    for (int k = 0; k < 3; k++) { g->support[2 * k] = (int16_t)(k < s.n ? s.x[k] : 0); g->support[2 * k + 1] = (int16_t)(k < s.n ? s.y[k] : 0); }
    circle_from_support(s, g->circle);
}

// a raw row -> the finished row; what the status says was not computed stays zero
static void finish_row(const vp_geom_raw& r, vp_contour_geom* g)
{
    memset(g, 0, sizeof *g);
    g->status = r.status & 0xffu;
    if (g->status & (GEOM_ST_SKIPPED | GEOM_ST_COORD)) return;
    if (!(g->status & GEOM_ST_PERIMETER)) {
        g->perimeter = (double)r.perim_units * (1.0 / GEOM_UNIT);
        g->perimeter_open = (double)(r.perim_units - vp_geom_root_units(r.close_root)) * (1.0 / GEOM_UNIT);
    }
    if (g->status & GEOM_ST_HULL_CAP) return;
    g->hull_count = r.hull_count;
    g->hull_area2 = r.hull_area2;
    if (r.hull_count == 1) {
        g->rect[0] = (float)r.edge[0]; g->rect[1] = (float)r.edge[1]; g->rect[4] = 90.f;
    } else if (r.hull_count >= 2) {
        const double ex = (double)r.edge[2] - (double)r.edge[0], ey = (double)r.edge[3] - (double)r.edge[1];
        const double ln = sqrt(ex * ex + ey * ey);
        const double ux = ex / ln, uy = ey / ln;
        double ext[4];
        for (int k = 0; k < 4; k++) {
            const double hx = (double)r.ext[2 * k], hy = (double)r.ext[2 * k + 1];
            ext[k] = k < 2 ? hx * ux + hy * uy : -hx * uy + hy * ux;
        }
        vp_min_area_rect_finish(r.edge[0], r.edge[1], r.edge[2], r.edge[3], ext, g->rect);
    }
    vp_geom_support s;
    s.n = (int)((r.status >> 8) & 3u);
    for (int k = 0; k < 3; k++) { s.x[k] = r.sup[2 * k]; s.y[k] = r.sup[2 * k + 1]; }
    store_support(s, g);
}

// the sequential loop of cv2_facade.arcLength (rows with GEOM_ST_PERIMETER)
static void perimeter_host(const int32_t* p, int n, double* closed, double* open)
{
    *closed = *open = 0.0;
    if (n <= 1) return;
    double total = 0.0;
    for (int i = 1; i < n; i++) total += (double)vp_geom_seg_root(p[2 * i] - p[2 * (i - 1)], p[2 * i + 1] - p[2 * (i - 1) + 1]);
    *open = total;
    double tc = 0.0;
    for (int i = 0; i < n; i++) {
        const int ip = i == 0 ? n - 1 : i - 1;
        tc += (double)vp_geom_seg_root(p[2 * i] - p[2 * ip], p[2 * i + 1] - p[2 * ip + 1]);
    }
    *closed = tc;
}

// hull, rectangle and circle of one contour by the host routines (rows with GEOM_ST_HULL_CAP); hull: room for n points
static int complete_row_host(const int32_t* p, int n, vp_contour_geom* g, int32_t* hull)
{
    int h = 0;
    if (vp_convex_hull_i32(p, n, hull, &h) != VP_OK) return VP_ERR_INVALID;
    long long a2 = 0;
    for (int i = 0; i < h; i++) {
        const int j = i + 1 == h ? 0 : i + 1;
        a2 += (long long)hull[2 * i] * hull[2 * j + 1] - (long long)hull[2 * j] * hull[2 * i + 1];
    }
    g->hull_count = h;
    g->hull_area2 = a2 < 0 ? -a2 : a2;
    if (vp_min_area_rect_i32(p, n, g->rect) != VP_OK) return VP_ERR_INVALID;
    vp_geom_support s;
    support_of_hull(hull, h, &s);
    store_support(s, g);
    return VP_OK;
}

static int fetch_rows(vp_ctx* ctx, const vp_geom_raw* d_rows, size_t n, vp_contour_geom* rows_out, const vp_geom_raw** raw_out)
{
    vp_geom_raw* raw = (vp_geom_raw*)vp_hstage(ctx, std::max<size_t>(n, 1) * sizeof(vp_geom_raw));
    if (!raw) return vp_fail(ctx, VP_ERR_NOMEM, "contour geometry: staging");
    if (n) VP_TRY(d2h(ctx, raw, d_rows, n * sizeof(vp_geom_raw)));
    VP_TRY(vp_synchronize(ctx));
    for (size_t i = 0; i < n; i++) finish_row(raw[i], rows_out + i);
    if (raw_out) *raw_out = raw;
    return VP_OK;
}

// the checks both flat entries share; n_points < 0: not known on the host
static int flat_refusal(vp_ctx* ctx, const void* pts, const void* counts, int n_contours, long long n_points, const void* rows)
{
    if (n_contours < 0) return vp_fail(ctx, VP_ERR_INVALID, "contour geometry: negative count");
    if (!rows && n_contours > 0) return vp_fail(ctx, VP_ERR_INVALID, "contour geometry: a pointer is missing");
    if (n_contours > 0 && (!counts || (n_points != 0 && !pts))) return vp_fail(ctx, VP_ERR_INVALID, "contour geometry: a pointer is missing");
    int code;
    if (const char* why = vp_geometry_refusal(n_contours, n_points < 0 ? 0 : n_points, &code)) return vp_fail(ctx, code, why);
    return VP_OK;
}

extern "C" {

int vp_contour_geometry_plan(int64_t n_contours, int64_t n_points, int want_hulls, uint64_t* ws_bytes, int32_t* grid3, int32_t* hull_cap)
{
    int code;
    if (const char* why = vp_geometry_refusal(n_contours, n_points, &code)) return vp_fail(nullptr, code, why);
    if (ws_bytes) *ws_bytes = vp_geometry_ws_bytes(n_contours, n_points, want_hulls != 0, 1);
    if (grid3) { grid3[0] = (int32_t)n_contours; grid3[1] = 1; grid3[2] = GEOM_TB; }
    if (hull_cap) *hull_cap = GEOM_HULL_CAP;
    return VP_OK;
}

int vp_min_enclosing_circle_i32(const int32_t* pts, int npts, float* out3, int32_t* support7)
{
    if (!out3 || npts < 0 || (npts > 0 && !pts)) return VP_ERR_INVALID;
    for (int i = 0; i < 2 * npts; i++)
        if (!vp_geometry_coord_ok(pts[i])) return vp_fail(nullptr, VP_ERR_UNSUPPORTED, "min enclosing circle: a coordinate outside [-32768, 32767]");
    std::vector<int32_t> hull((size_t)std::max(npts, 1) * 2);
    int h = 0;
    if (npts > 0 && vp_convex_hull_i32(pts, npts, hull.data(), &h) != VP_OK) return VP_ERR_INVALID;
    vp_geom_support s;
    support_of_hull(hull.data(), h, &s);
    circle_from_support(s, out3);
    if (support7) {
        support7[0] = s.n;
        for (int k = 0; k < 3; k++) { support7[1 + 2 * k] = k < s.n ? s.x[k] : 0; support7[2 + 2 * k] = k < s.n ? s.y[k] : 0; }
    }
    return VP_OK;
}

int vp_contour_geometry_i32(vp_ctx* ctx, const int32_t* pts, const int32_t* counts, int n_contours, vp_contour_geom* rows_out, int32_t* hull_pts_out,
                            int32_t* hull_counts_out)
{
    if (n_contours < 0) return vp_fail(ctx, VP_ERR_INVALID, "contour geometry: negative count");
    if (n_contours > 0 && !counts) return vp_fail(ctx, VP_ERR_INVALID, "contour geometry: a pointer is missing");
    long long total = 0;
    for (int i = 0; i < n_contours; i++) {
        if (counts[i] < 0) return vp_fail(ctx, VP_ERR_INVALID, "contour geometry: negative count");
        total += counts[i];
    }
    VP_TRY(flat_refusal(ctx, pts, counts, n_contours, total, rows_out));
    for (long long i = 0; i < 2 * total; i++)
        if (!vp_geometry_coord_ok(pts[i])) return vp_fail(ctx, VP_ERR_UNSUPPORTED, "contour geometry: a coordinate outside [-32768, 32767]");
    VP_TRY(check_ctx(ctx));
    if (n_contours == 0) return VP_OK;
    const size_t n = (size_t)n_contours, np = (size_t)total;
    vp_ws_frame W;
    int32_t* d_pts; W.want(&d_pts, std::max<size_t>(np, 1) * 8);
    long long* d_first; W.want(&d_first, n * 8);
    int32_t* d_counts; W.want(&d_counts, n * 4);
    vp_geom_raw* d_rows; W.want(&d_rows, n * sizeof(vp_geom_raw));
    int32_t* d_hull = nullptr;
    if (hull_pts_out) W.want(&d_hull, std::max<size_t>(np, 1) * 8);
    VP_TRY(vp_ws_commit(ctx, W, "vp_contour_geometry_i32"));
    std::vector<long long> first(n);
    long long at = 0;
    for (size_t i = 0; i < n; i++) { first[i] = at; at += counts[i]; }
    if (np) VP_TRY(h2d(ctx, d_pts, pts, np * 8));
    VP_TRY(h2d(ctx, d_first, first.data(), n * 8));
    VP_TRY(h2d(ctx, d_counts, counts, n * 4));
    VP_TRY(vpk_contour_geometry(ctx, d_pts, d_first, d_counts, n_contours, d_rows, d_hull));
    if (d_hull && np) VP_TRY(d2h(ctx, hull_pts_out, d_hull, np * 8));
    VP_TRY(fetch_rows(ctx, d_rows, n, rows_out, nullptr));    // synchronises: `first` and the hull block are done with
    std::vector<int32_t> tmp;
    for (size_t i = 0; i < n; i++) {
        vp_contour_geom* g = rows_out + i;
        const int32_t* p = pts + 2 * first[i];
        if (g->status & GEOM_ST_PERIMETER) perimeter_host(p, counts[i], &g->perimeter, &g->perimeter_open);
        if (g->status & GEOM_ST_HULL_CAP) {
            int32_t* hull = hull_pts_out ? hull_pts_out + 2 * first[i] : (tmp.resize((size_t)counts[i] * 2), tmp.data());
            VP_TRY(complete_row_host(p, counts[i], g, hull));
        }
        if (hull_counts_out) hull_counts_out[i] = g->hull_count;
    }
    return VP_OK;
}

int vp_contour_geometry_dev(vp_ctx* ctx, const int32_t* d_pts, const int64_t* d_first, const int32_t* d_counts, int n_contours, vp_contour_geom* rows_out,
                            int32_t* d_hull)
{
    VP_TRY(flat_refusal(ctx, d_pts, d_counts, n_contours, -1, rows_out));
    if (n_contours > 0 && !d_first) return vp_fail(ctx, VP_ERR_INVALID, "contour geometry: a pointer is missing");
    if ((uintptr_t)d_pts % 8 || (uintptr_t)d_first % 8 || (uintptr_t)d_counts % 4 || (uintptr_t)d_hull % 8)
        return vp_fail(ctx, VP_ERR_INVALID, "contour geometry: points and first indices must be 8-byte aligned");
    VP_TRY(check_ctx(ctx));
    if (n_contours == 0) return VP_OK;
    vp_ws_frame W;
    vp_geom_raw* d_rows; W.want(&d_rows, (size_t)n_contours * sizeof(vp_geom_raw));
    VP_TRY(vp_ws_commit(ctx, W, "vp_contour_geometry_dev"));
    VP_TRY(vpk_contour_geometry(ctx, d_pts, reinterpret_cast<const long long*>(d_first), d_counts, n_contours, d_rows, d_hull));
    return fetch_rows(ctx, d_rows, (size_t)n_contours, rows_out, nullptr);
}

int vp_contour_geometry_batch_dev(vp_ctx* ctx, const vp_contour_desc* cd, const vp_contour_buffers* cb, int n_frames, vp_contour_geom* rows_out)
{
    if (!cd || !cb || !rows_out) return vp_fail(ctx, VP_ERR_INVALID, "contour geometry: a pointer is missing");
    if (n_frames < 0 || n_frames > 65535) return vp_fail(ctx, VP_ERR_INVALID, "contour geometry: 0..65535 frames");
    if (cd->max_contours <= 0 || cd->max_points <= 0) return vp_fail(ctx, VP_ERR_INVALID, "contours: capacity");
    if (!cb->info || !cb->counts || !cb->offsets || !cb->points) return vp_fail(ctx, VP_ERR_INVALID, "contour geometry: a pointer is missing");
    if ((uintptr_t)cb->points % 8) return vp_fail(ctx, VP_ERR_INVALID, "contour geometry: points must be 8-byte aligned");
    int code;
    if (const char* why = vp_geometry_refusal((long long)cd->max_contours * n_frames, cd->max_points, &code)) return vp_fail(ctx, code, why);
    VP_TRY(check_ctx(ctx));
    if (n_frames == 0) return VP_OK;
    const size_t n = (size_t)cd->max_contours * n_frames;
    vp_ws_frame W;
    vp_geom_raw* d_rows; W.want(&d_rows, n * sizeof(vp_geom_raw));
    VP_TRY(vp_ws_commit(ctx, W, "vp_contour_geometry_batch_dev"));
    VP_TRY(vpk_contour_geometry_batch(ctx, cb->info, cb->counts, cb->offsets, cb->points, n_frames, cd->max_contours, cd->max_points, d_rows));
    return fetch_rows(ctx, d_rows, n, rows_out, nullptr);
}

}  // extern "C"
