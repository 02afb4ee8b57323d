// C ABI of libvp.so, shapes: polygon sums, convex hull, minimum-area rectangle and the overlay rasteriser on the host, the
// overlay, filled shapes and cv2.addWeighted on device images (kernels: vp_morph, vp_fill).
#include "vp_api_util.h"
#include "vp_geometry_plan.h"

// The tail of the calipers, for every path that has found its edge (vp_min_area_rect_i32 below, the rows of the device pass in
// vp_api_geometry.hip): the edge (x0, y0) -> (x1, y1), of length above 0, and the four extents amax, amin, bmax, bmin along and across
// it -> centre, sizes, the angle and its swap loop, rounded to float once.
void vp_min_area_rect_finish(int x0, int y0, int x1, int y1, const double* ext4, float* out5)
{
    const double ex = (double)x1 - (double)x0, ey = (double)y1 - (double)y0;
    const double ln = sqrt(ex * ex + ey * ey);
    const double ux = ex / ln, uy = ey / ln;
    const double amax = ext4[0], amin = ext4[1], bmax = ext4[2], bmin = ext4[3];
    double bwd = amax - amin, bht = bmax - bmin;
    const double ca = (amax + amin) / 2, cb = (bmax + bmin) / 2;
    const double bcx = ca * ux - cb * uy, bcy = ca * uy + cb * ux;
    double bang = atan2(uy, ux) * (180.0 / 3.141592653589793);
    while (bang <= 0) { bang += 90; std::swap(bwd, bht); }
    while (bang > 90) { bang -= 90; std::swap(bwd, bht); }
    out5[0] = (float)bcx; out5[1] = (float)bcy; out5[2] = (float)bwd; out5[3] = (float)bht; out5[4] = (float)bang;
}

extern "C" {

// ---- debug overlays (host only, no device work) -----------------------------------------------------------------------------
// utils/draw.py:283-327 draw_contours / draw_polylines modify the caller's host image in place on every frame
// (modules/red_buoy.py:39).  The Python mirror's rasteriser (Bresenham steps, square brush of the requested thickness) is the
// same statement sequence here in C, because at 1080p a dozen contours of a few hundred points are 10^4 brush stamps per frame.
// utils/feature.py:240-265 contour_centroid / contour_area (cv2.moments, cv2.contourArea on an integer contour): the three Green sums
// a00 = sum(x[i-1] y[i] - x[i] y[i-1]), a10 = sum(d (x[i-1] + x[i])), a01 = sum(d (y[i-1] + y[i])) as exact integers (host code).
int vp_polygon_sums_i32(const int32_t* pts, int npts, int64_t* out3)
{
    if (!pts || !out3 || npts < 0) return VP_ERR_INVALID;
    long long a00 = 0, a10 = 0, a01 = 0;
    if (npts > 0) {
        long long xp = pts[2 * (npts - 1)], yp = pts[2 * (npts - 1) + 1];
        for (int i = 0; i < npts; i++) {
            const long long x = pts[2 * i], y = pts[2 * i + 1];
            const long long d = xp * y - x * yp;
            a00 += d; a10 += d * (xp + x); a01 += d * (yp + y);
            xp = x; yp = y;
        }
    }
    out3[0] = a00; out3[1] = a10; out3[2] = a01;
    return VP_OK;
}

// Convex hull of integer points (host code; cv2.minAreaRect of the stand-in, modules/bins.py:62): Andrew's monotone chain over the
// sorted distinct points, collinear points dropped, counter-clockwise from the lexicographically smallest point - exact in 64-bit
// integers.  out must hold npts points; returns the number of hull vertices in *nout.
int vp_convex_hull_i32(const int32_t* pts, int npts, int32_t* out, int* nout)
{
    if (!pts || !out || !nout || npts < 0) return VP_ERR_INVALID;
    std::vector<std::pair<int32_t, int32_t>> p((size_t)npts);
    for (int i = 0; i < npts; i++) p[(size_t)i] = {pts[2 * i], pts[2 * i + 1]};
    std::sort(p.begin(), p.end());
    p.erase(std::unique(p.begin(), p.end()), p.end());
    const int n = (int)p.size();
    if (n <= 2) {
        for (int i = 0; i < n; i++) { out[2 * i] = p[(size_t)i].first; out[2 * i + 1] = p[(size_t)i].second; }
        *nout = n;
        return VP_OK;
    }
    auto cross = [](const std::pair<int32_t, int32_t>& o, const std::pair<int32_t, int32_t>& a, const std::pair<int32_t, int32_t>& b) {
        return ((long long)a.first - o.first) * ((long long)b.second - o.second) - ((long long)a.second - o.second) * ((long long)b.first - o.first);
    };
    std::vector<std::pair<int32_t, int32_t>> lower, upper;
    for (int i = 0; i < n; i++) {
        while (lower.size() >= 2 && cross(lower[lower.size() - 2], lower.back(), p[(size_t)i]) <= 0) lower.pop_back();
        lower.push_back(p[(size_t)i]);
    }
    for (int i = n - 1; i >= 0; i--) {
        while (upper.size() >= 2 && cross(upper[upper.size() - 2], upper.back(), p[(size_t)i]) <= 0) upper.pop_back();
        upper.push_back(p[(size_t)i]);
    }
    int k = 0;
    for (size_t i = 0; i + 1 < lower.size(); i++, k++) { out[2 * k] = lower[i].first; out[2 * k + 1] = lower[i].second; }
    for (size_t i = 0; i + 1 < upper.size(); i++, k++) { out[2 * k] = upper[i].first; out[2 * k + 1] = upper[i].second; }
    *nout = k;
    return VP_OK;
}

// cv2.minAreaRect of the stand-in for integer points (host code; modules/bins.py:62 calls it for every contour): rotating calipers
// over the hull above - for every hull edge the extent of the hull along and across it, the first edge of smallest area wins -
// in the doubles of the Python statements (vision/cv2_facade.py _min_area_rect_loop; edge lengths as sqrt of an exact integer).
// out5 = cx, cy, width, height, angle in degrees (OpenCV >= 4.5.1 convention: angle in (0, 90]), already rounded to float.
int vp_min_area_rect_i32(const int32_t* pts, int npts, float* out5)
{
    if (!pts || !out5 || npts < 0) return VP_ERR_INVALID;
    std::vector<int32_t> hull((size_t)std::max(npts, 1) * 2);
    int n = 0;
    if (vp_convex_hull_i32(pts, npts, hull.data(), &n) != VP_OK) return VP_ERR_INVALID;
    if (n == 0) { for (int i = 0; i < 5; i++) out5[i] = 0.f; return VP_OK; }
    if (n == 1) { out5[0] = (float)hull[0]; out5[1] = (float)hull[1]; out5[2] = out5[3] = 0.f; out5[4] = 90.f; return VP_OK; }
    int best = -1;
    double best_area = 0, best_ext[4] = {0, 0, 0, 0};
    const vp_geom_hull_i32 H = {hull.data()};
    const int edges = n > 2 ? n : 1;
    for (int i = 0; i < edges; i++) {
        double ext[4];
        int arg[4];
        if (!vp_geom_edge_extents(H, n, i, ext, arg)) continue;
        const double wd = ext[0] - ext[1], ht = ext[2] - ext[3];
        if (best < 0 || wd * ht < best_area) {
            best = i;
            best_area = wd * ht;
            for (int k = 0; k < 4; k++) best_ext[k] = ext[k];
        }
    }
    if (best < 0) { out5[0] = (float)hull[0]; out5[1] = (float)hull[1]; out5[2] = out5[3] = 0.f; out5[4] = 90.f; return VP_OK; }
    const int b1 = (best + 1) % n;
    vp_min_area_rect_finish(hull[2 * best], hull[2 * best + 1], hull[2 * b1], hull[2 * b1 + 1], best_ext, out5);
    return VP_OK;
}

// counts[k] points per polyline, back to back in pts; one call draws them all (a frame's contours).
// All stamps carry one colour, so the image is "colour wherever some stamp covers": the stamps are collected in a coverage bit plane
// (one bit per pixel, 259 KB at 1080p, per thread, left zeroed) and the image is written once, row by row, run by run.
// filled (vp_fill_polys_u8; the caller has checked the coordinate bound): the even-odd spans of every polygon enter the plane first.
static int raster_polys_u8(uint8_t* img, size_t stride, int w, int h, int cn, const int32_t* pts, const int32_t* counts, int npolys, int closed,
                           const uint8_t* color, int thickness, bool filled)
{
    if (thickness < 1) thickness = 1;
    const int r0 = (thickness - 1) / 2, r1 = thickness / 2;
    const int ww = (w + 63) >> 6;
    static thread_local std::vector<uint64_t> cover;
    if (cover.size() < (size_t)ww * h) cover.assign((size_t)ww * h, 0);
    uint64_t* cv = cover.data();
    int ylo = h, yhi = -1, wlo = ww, whi = -1;              // rows / words touched
    auto span = [&](int y, int xa, int xb) {               // bits [xa, xb) of row y; the caller has clipped y
        xa = std::max(xa, 0); xb = std::min(xb, w);
        if (xa >= xb) return;
        uint64_t* row = cv + (size_t)y * ww;
        const int wa = xa >> 6, wb = (xb - 1) >> 6;
        const uint64_t ma = ~0ull << (xa & 63), mb = ~0ull >> (63 - ((xb - 1) & 63));
        if (wa == wb) row[wa] |= ma & mb;
        else { row[wa] |= ma; for (int k = wa + 1; k < wb; k++) row[k] = ~0ull; row[wb] |= mb; }
        wlo = std::min(wlo, wa); whi = std::max(whi, wb);
    };
    auto fill = [&](int xa, int xb, int ya, int yb) {      // [xa, xb) x [ya, yb), clipped
        ya = std::max(ya, 0); yb = std::min(yb, h);
        if (ya >= yb || xb <= 0 || xa >= w) return;
        ylo = std::min(ylo, ya); yhi = std::max(yhi, yb - 1);
        for (int yy = ya; yy < yb; yy++) span(yy, xa, xb);
    };
    auto column = [&](int x, int ya, int yb) {             // one pixel wide: the strip a horizontal step adds
        ya = std::max(ya, 0); yb = std::min(yb, h);
        if (ya >= yb || x < 0 || x >= w) return;
        ylo = std::min(ylo, ya); yhi = std::max(yhi, yb - 1);
        const int k = x >> 6;
        wlo = std::min(wlo, k); whi = std::max(whi, k);
        const uint64_t bit = 1ull << (x & 63);
        uint64_t* q = cv + (size_t)ya * ww + k;
        for (int yy = ya; yy < yb; yy++, q += ww) *q |= bit;
    };
    // The brush is a square stamped at every Bresenham step.  A step moves by at most one pixel per axis, so the square at the new
    // position adds one column and / or one row to what the previous stamp covered: only that strip is marked.
    bool have = false;
    int lx = 0, ly = 0;
    auto stamp = [&](int x, int y) {
        if (have && x == lx && y == ly) return;
        if (have && abs(x - lx) <= 1 && abs(y - ly) <= 1) {
            if (x != lx) { const int cx = x > lx ? x + r1 : x - r0; column(cx, y - r0, y + r1 + 1); }
            if (y != ly) { const int cy = y > ly ? y + r1 : y - r0; fill(x - r0, x + r1 + 1, cy, cy + 1); }
        } else {
            fill(x - r0, x + r1 + 1, y - r0, y + r1 + 1);
        }
        have = true; lx = x; ly = y;
    };
    auto line = [&](int x0, int y0, int x1, int y1) {
        if (y0 == y1 && abs(x1 - x0) > 2) {                 // a horizontal run (straight stretches of a simplified contour): one box
            fill(std::min(x0, x1) - r0, std::max(x0, x1) + r1 + 1, y0 - r0, y0 + r1 + 1);
            have = true; lx = x1; ly = y1;
            return;
        }
        const int dx = abs(x1 - x0), dy = -abs(y1 - y0);
        const int sx = x0 < x1 ? 1 : -1, sy = y0 < y1 ? 1 : -1;
        long long err = (long long)dx + dy;
        for (;;) {
            stamp(x0, y0);
            if (x0 == x1 && y0 == y1) break;
            const long long e2 = 2 * err;
            if (e2 >= dy) { err += dy; x0 += sx; }
            if (e2 <= dx) { err += dx; y0 += sy; }
        }
    };
    // vision/utils/draw.py _fill: rows of the clipped bounding box; an edge counts on row y when min(ya, yb) <= y < max(ya, yb); the
    // sorted crossings pair up into spans [ceil(a), floor(b)].  The edges are taken in the order of their first row and kept in a list
    // while the sweep is inside them; the crossings are exact keys (vp_fill_cross_key), any number of them per row.
    static thread_local std::vector<int> order, active;
    static thread_local std::vector<u64> keys;
    auto fill_poly = [&](const int32_t* p, int n) {
        int ymin = p[1], ymax = p[1];
        for (int i = 1; i < n; i++) { ymin = std::min(ymin, p[2 * i + 1]); ymax = std::max(ymax, p[2 * i + 1]); }
        const int y0 = std::max(ymin, 0), y1 = std::min(ymax, h - 1);
        if (y0 > y1 || ymin == ymax) return;
        auto first_row = [&](int e) { int lo, hi; vp_fill_edge_rows(p[2 * e + 1], p[2 * (e + 1 == n ? 0 : e + 1) + 1], &lo, &hi); return lo; };
        auto end_row = [&](int e) { int lo, hi; vp_fill_edge_rows(p[2 * e + 1], p[2 * (e + 1 == n ? 0 : e + 1) + 1], &lo, &hi); return hi; };
        order.clear();
        for (int e = 0; e < n; e++) { int lo, hi; if (vp_fill_edge_rows(p[2 * e + 1], p[2 * (e + 1 == n ? 0 : e + 1) + 1], &lo, &hi)) order.push_back(e); }
        std::sort(order.begin(), order.end(), [&](int a, int b) { return first_row(a) < first_row(b); });
        active.clear();
        size_t next = 0;
        for (int y = y0; y <= y1; y++) {
            for (; next < order.size() && first_row(order[next]) <= y; next++) active.push_back(order[next]);
            keys.clear();
            for (size_t i = 0; i < active.size();) {
                const int e = active[i], e1 = e + 1 == n ? 0 : e + 1;
                if (end_row(e) <= y) { active[i] = active.back(); active.pop_back(); continue; }
                keys.push_back(vp_fill_cross_key(p[2 * e], p[2 * e + 1], p[2 * e1], p[2 * e1 + 1], y));
                i++;
            }
            std::sort(keys.begin(), keys.end());
            for (size_t i = 0; i + 1 < keys.size(); i += 2) fill(vp_fill_key_ceil(keys[i]), vp_fill_key_floor(keys[i + 1]) + 1, y, y + 1);
        }
    };
    size_t o = 0;
    int rc = VP_OK;
    for (int k = 0; k < npolys; k++) {
        const int npts = counts[k];
        if (npts < 0) { rc = VP_ERR_INVALID; break; }
        const int32_t* p = pts + 2 * o;
        o += (size_t)npts;
        have = false;
        if (npts == 0) continue;
        if (filled) fill_poly(p, npts);
        if (npts == 1) { line(p[0], p[1], p[0], p[1]); continue; }
        const int last = closed ? npts : npts - 1;
        for (int i = 0; i < last; i++) {
            const int j = i + 1 < npts ? i + 1 : 0;
            line(p[2 * i], p[2 * i + 1], p[2 * j], p[2 * j + 1]);
        }
    }
    // write the covered pixels, run by run, and hand the plane back zeroed (also after an error)
    const uint8_t c0 = color[0], c1 = color[cn > 1 ? 1 : 0], c2 = color[cn > 2 ? 2 : 0];
    // The caller's image has usually just been written by a 6 MB copy and is not in the core's cache: every run below would wait for
    // its line.  The plane says which lines those are, so they are requested some rows ahead of the writes (MI355X host, one frame's
    // contours at 1080p, thickness 10: 115 -> 57 us; stamping strips straight into the image: 93 us).
    auto prefetch_row = [&](int y) {
        if (y > yhi) return;
        const uint64_t* row = cv + (size_t)y * ww;
        const uint8_t* out = img + (size_t)y * stride;
        for (int k = wlo; k <= whi; k++) {
            uint64_t m = row[k];
            if (!m) continue;
            const int a = __builtin_ctzll(m), b = 63 - __builtin_clzll(m);
            const uint8_t* q0 = out + ((size_t)k * 64 + a) * cn;
            const uint8_t* q1 = out + ((size_t)k * 64 + b) * cn + cn - 1;
            for (const uint8_t* q = (const uint8_t*)((uintptr_t)q0 & ~(uintptr_t)63); q <= q1; q += 64) __builtin_prefetch(q, 1, 3);
        }
    };
    for (int y = ylo; y < ylo + 16; y++) prefetch_row(y);
    for (int y = ylo; y <= yhi; y++) {
        prefetch_row(y + 16);
        uint64_t* row = cv + (size_t)y * ww;
        uint8_t* out = img + (size_t)y * stride;
        for (int k = wlo; k <= whi; k++) {
            uint64_t m = row[k];
            if (!m) continue;
            row[k] = 0;
            if (rc != VP_OK) continue;
            while (m) {
                const int a = __builtin_ctzll(m);
                const uint64_t rest = ~(m >> a);            // first zero above a = end of the run
                const int len = rest ? __builtin_ctzll(rest) : 64 - a;
                uint8_t* q = out + ((size_t)k * 64 + a) * cn;
                if (cn == 3) for (int i = 0; i < len; i++, q += 3) { q[0] = c0; q[1] = c1; q[2] = c2; }
                else if (cn == 1) memset(q, c0, (size_t)len);
                else for (int i = 0; i < len; i++, q += cn) memcpy(q, color, (size_t)cn);
                if (a + len >= 64) break;
                m &= ~0ull << (a + len);
            }
        }
    }
    return rc;
}

int vp_draw_polylines_u8(uint8_t* img, size_t stride, int w, int h, int cn, const int32_t* pts, const int32_t* counts, int npolys, int closed,
                         const uint8_t* color, int thickness)
{
    if (!img || !pts || !counts || !color || w <= 0 || h <= 0 || cn < 1 || cn > 4 || npolys < 0 || stride < (size_t)w * cn) return VP_ERR_INVALID;
    return raster_polys_u8(img, stride, w, h, cn, pts, counts, npolys, closed, color, thickness, false);
}

int vp_draw_polyline_u8(uint8_t* img, size_t stride, int w, int h, int cn, const int32_t* pts, int npts, int closed, const uint8_t* color,
                        int thickness)
{
    const int32_t cnt = npts;
    return vp_draw_polylines_u8(img, stride, w, h, cn, pts, &cnt, 1, closed, color, thickness);
}

// The polylines of vp_draw_polylines_u8 drawn into a packed device image (bins.py draws its rectangles into an overlay that only ever
// leaves the device when it is posted).  Points and counts are host arrays; the same pixels as the host rasteriser.
// fill (nullable; vp_fill_polys_dev): the polygons' rows, filled on the same stream before the outline - the descriptors travel with
// the vertices.
static int polylines_dev(vp_ctx* ctx, const char* who, uint8_t* d_img, int w, int h, int cn, const int32_t* pts, const int32_t* counts, int npolys, int closed,
                         const uint8_t* color, int thickness, long long total, const std::vector<vp_fill_poly>* fill, int fill_rows)
{
    // the vertices and, per vertex, the vertex it is joined to go over in one pinned chunk; the device walks the lines (k_draw_segments)
    if (total == 0) return VP_OK;
    if (total > (1ll << 28)) return vp_fail(ctx, VP_ERR_INVALID, who);
    const size_t N = (size_t)total;
    const size_t nfill = fill ? fill->size() : 0;
    auto link = [&](int32_t* nx) {                       // per vertex, the vertex it is joined to (-1: the open end of a polyline)
        size_t o = 0;
        for (int k = 0; k < npolys; k++) {
            const size_t npts = (size_t)counts[k];
            for (size_t i = 0; i + 1 < npts; i++) nx[o + i] = (int32_t)(o + i + 1);
            if (npts) nx[o + npts - 1] = (npts == 1 || closed) ? (int32_t)o : -1;
            o += npts;
        }
    };
    if (N <= 48 && nfill <= VP_FILL_SMALL_POLYS) {       // a few vertices travel as kernel arguments (vpk_draw_small)
        int32_t nx[48];
        link(nx);
        if (nfill) VP_TRY(vpk_fill_polys(ctx, d_img, w, h, cn, pts, (int)N, fill->data(), (int)nfill, fill_rows, color, true));
        return vpk_draw_small(ctx, d_img, w, h, cn, pts, nx, (int)N, thickness, color);
    }
    const size_t fill_off = vp_align(N * 12, 16), bytes = fill_off + nfill * sizeof(vp_fill_poly);
    int slot = -1;
    uint8_t* hp = vp_ring_take(ctx, bytes, &slot);
    if (!hp) return vp_fail(ctx, VP_ERR_NOMEM, "pinned staging");
    memcpy(hp, pts, N * 8);
    link(reinterpret_cast<int32_t*>(hp + N * 8));
    if (nfill) memcpy(hp + fill_off, fill->data(), nfill * sizeof(vp_fill_poly));
    vp_ws_frame W;
    uint8_t* d_buf; W.want(&d_buf, bytes);
    int rc = vp_ws_commit(ctx, W, "overlay vertices");
    if (rc == VP_OK) rc = h2d(ctx, d_buf, hp, bytes);
    if (rc == VP_OK && nfill)
        rc = vpk_fill_polys(ctx, d_img, w, h, cn, reinterpret_cast<const int32_t*>(d_buf), (int)N, reinterpret_cast<const vp_fill_poly*>(d_buf + fill_off), (int)nfill,
                            fill_rows, color, false);
    if (rc == VP_OK)
        rc = vpk_draw_segments(ctx, d_img, w, h, cn, reinterpret_cast<const int32_t*>(d_buf), reinterpret_cast<const int32_t*>(d_buf + N * 8), (int)N, thickness, color);
    vp_ring_done(ctx, slot);
    return rc;
}

int vp_draw_polylines_dev(vp_ctx* ctx, uint8_t* d_img, int w, int h, int cn, const int32_t* pts, const int32_t* counts, int npolys, int closed,
                          const uint8_t* color, int thickness)
{
    VP_TRY(check_ctx(ctx));
    if (!d_img || !pts || !counts || !color || w <= 0 || h <= 0 || cn < 1 || cn > 4 || npolys < 0) return vp_fail(ctx, VP_ERR_INVALID, "vp_draw_polylines_dev arguments");
    if (thickness < 1) thickness = 1;
    if (thickness > 255) return vp_fail(ctx, VP_ERR_UNSUPPORTED, "vp_draw_polylines_dev: thickness");
    long long total = 0;
    for (int k = 0; k < npolys; k++) {
        if (counts[k] < 0) return vp_fail(ctx, VP_ERR_INVALID, "vp_draw_polylines_dev: counts");
        total += counts[k];
    }
    return polylines_dev(ctx, "vp_draw_polylines_dev: too many points", d_img, w, h, cn, pts, counts, npolys, closed, color, thickness, total, nullptr, 0);
}

// ---- filled polygons, rectangles and discs --------------------------------------------------------------------------------------
// The checks vp_fill_polys_u8 and vp_fill_polys_dev share (ctx is NULL for the host form): the arguments of the outline entries, then
// the coordinate bound under which the integer crossings are the float64 crossings of the Python statement.
static int fill_polys_args(vp_ctx* ctx, const char* who, const void* img, int w, int h, int cn, const int32_t* pts, const int32_t* counts, int npolys,
                           const uint8_t* color, long long* total)
{
    if (!img || !pts || !counts || !color || w <= 0 || h <= 0 || cn < 1 || cn > 4 || npolys < 0) return vp_fail(ctx, VP_ERR_INVALID, who);
    long long n = 0;
    for (int k = 0; k < npolys; k++) {
        if (counts[k] < 0) return vp_fail(ctx, VP_ERR_INVALID, who);
        n += counts[k];
    }
    if (n > (1ll << 28)) return vp_fail(ctx, VP_ERR_INVALID, who);
    for (long long i = 0; i < 2 * n; i++)
        if (pts[i] > VP_FILL_MAX_COORD || pts[i] < -VP_FILL_MAX_COORD) return vp_fail(ctx, VP_ERR_UNSUPPORTED, "filled polygon: a coordinate beyond VP_FILL_MAX_COORD");
    *total = n;
    return VP_OK;
}

int vp_fill_polys_u8(uint8_t* img, size_t stride, int w, int h, int cn, const int32_t* pts, const int32_t* counts, int npolys, const uint8_t* color)
{
    long long total = 0;
    VP_TRY(fill_polys_args(nullptr, "vp_fill_polys_u8 arguments", img, w, h, cn, pts, counts, npolys, color, &total));
    if (stride < (size_t)w * cn) return vp_fail(nullptr, VP_ERR_INVALID, "vp_fill_polys_u8 arguments");
    return raster_polys_u8(img, stride, w, h, cn, pts, counts, npolys, 1, color, 1, true);
}

int vp_fill_polys_dev(vp_ctx* ctx, uint8_t* d_img, int w, int h, int cn, const int32_t* pts, const int32_t* counts, int npolys, const uint8_t* color)
{
    VP_TRY(check_ctx(ctx));
    long long total = 0;
    VP_TRY(fill_polys_args(ctx, "vp_fill_polys_dev arguments", d_img, w, h, cn, pts, counts, npolys, color, &total));
    // per polygon its clipped rows, and the crossings of every one of them counted here (an edge adds one to each row from its upper end
    // to just above its lower end: a difference array), so that a row the kernel could not sort is known before anything is enqueued
    static thread_local std::vector<vp_fill_poly> polys;
    static thread_local std::vector<int> diff;
    polys.clear();
    long long rows = 0;
    size_t o = 0;
    for (int k = 0; k < npolys; k++) {
        const int n = counts[k];
        const int32_t* p = pts + 2 * o;
        const size_t first = o;
        o += (size_t)n;
        if (n < 2) continue;
        int ymin = p[1], ymax = p[1];
        for (int i = 1; i < n; i++) { ymin = std::min(ymin, p[2 * i + 1]); ymax = std::max(ymax, p[2 * i + 1]); }
        const int y0 = std::max(ymin, 0), y1 = std::min(ymax, h - 1);
        if (y0 > y1 || ymin == ymax) continue;
        diff.assign((size_t)(y1 - y0 + 2), 0);
        for (int i = 0; i < n; i++) {
            int lo, hi;
            if (!vp_fill_edge_rows(p[2 * i + 1], p[2 * (i + 1 == n ? 0 : i + 1) + 1], &lo, &hi)) continue;
            lo = std::max(lo, y0); hi = std::min(hi, y1 + 1);
            if (lo < hi) { diff[(size_t)(lo - y0)]++; diff[(size_t)(hi - y0)]--; }
        }
        int run = 0;
        for (int y = y0; y <= y1; y++) {
            run += diff[(size_t)(y - y0)];
            if (run > VP_FILL_MAX_CROSS) return vp_fail(ctx, VP_ERR_CAPACITY, "vp_fill_polys_dev: a row with more than VP_FILL_MAX_CROSS crossings");
        }
        polys.push_back(vp_fill_poly{(int32_t)first, n, y0, y1 - y0 + 1, (int32_t)rows});
        rows += y1 - y0 + 1;
        if (rows > (1ll << 30)) return vp_fail(ctx, VP_ERR_UNSUPPORTED, "vp_fill_polys_dev: too many rows");
    }
    return polylines_dev(ctx, "vp_fill_polys_dev arguments", d_img, w, h, cn, pts, counts, npolys, 1, color, 1, total, &polys, (int)rows);
}

// draw_rect / draw_circle with a negative thickness (vision/utils/draw.py): the numpy slices, written by the device
static int fill_shape_args(vp_ctx* ctx, const char* who, const void* img, int w, int h, int cn, const uint8_t* color, int a, int b, int c, int d)
{
    if (!img || !color || w <= 0 || h <= 0 || cn < 1 || cn > 4) return vp_fail(ctx, VP_ERR_INVALID, who);
    const int lim = 1 << 20;
    if (a > lim || a < -lim || b > lim || b < -lim || c > lim || c < -lim || d > lim || d < -lim) return vp_fail(ctx, VP_ERR_UNSUPPORTED, "filled shape: a coordinate beyond 2^20");
    return VP_OK;
}

int vp_fill_rect_dev(vp_ctx* ctx, uint8_t* d_img, int w, int h, int cn, int x0, int y0, int x1, int y1, const uint8_t* color)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(fill_shape_args(ctx, "vp_fill_rect_dev arguments", d_img, w, h, cn, color, x0, y0, x1, y1));
    const int xa = std::max(std::min(x0, x1), 0), xb = std::min(std::max(x0, x1), w - 1);
    const int ya = std::max(std::min(y0, y1), 0), yb = std::min(std::max(y0, y1), h - 1);
    if (xa > xb || ya > yb) return VP_OK;
    return vpk_fill_rect(ctx, d_img, w, h, cn, xa, xb, ya, yb, color);
}

int vp_fill_circle_dev(vp_ctx* ctx, uint8_t* d_img, int w, int h, int cn, int cx, int cy, int radius, const uint8_t* color)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(fill_shape_args(ctx, "vp_fill_circle_dev arguments", d_img, w, h, cn, color, cx, cy, radius, 0));
    if (radius < 0) return VP_OK;
    return vpk_fill_disc(ctx, d_img, w, h, cn, cx, cy, radius, color);
}

// cv2.addWeighted on two device images of n bytes each (modules/bins.py:20: the mask overlay); d_dst may be one of the sources
int vp_add_weighted_u8_dev(vp_ctx* ctx, const uint8_t* d_a, double alpha, const uint8_t* d_b, double beta, double gamma, size_t n, uint8_t* d_dst)
{
    VP_TRY(check_ctx(ctx));
    if (!d_a || !d_b || !d_dst || n == 0 || n > ((size_t)1 << 40)) return vp_fail(ctx, VP_ERR_INVALID, "vp_add_weighted_u8_dev arguments");
    return vpk_add_weighted_u8(ctx, d_a, d_b, n, alpha, beta, gamma, d_dst);
}

}  // extern "C"
