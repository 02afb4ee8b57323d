// Size rules, refusals, row layouts and the exact predicates of the contour-geometry pass (vp_geometry.hip), shared with the C ABI
// (vp_api_geometry.hip, vp_api_shapes.hip); the tests read the numbers from this file.  Everything here is decided on the host before
// a launch: the launches depend on the data only through the status word of a row.
//
// Coordinates.  Points are int32 (x, y) with both coordinates in [GEOM_COORD_MIN, GEOM_COORD_MAX] - every image find_contours accepts.
// Differences then fit 17 bits, squared lengths 33 bits, the in-circle determinant 128 bits; a point packs into 32 bits, x high, so that
// unsigned order of the packed words is lexicographic order of the points.
//
// Perimeter.  A segment's length is the float32 root of the float32 dx*dx + dy*dy (cv2_facade.arcLength).  For lattice points every
// such root is 0 or at least 1, below 2^17, and so a multiple of 2^-23: root * 2^23 is an integer below 2^40.  The pass adds these
// integers in 64 bits, in any order.  While the total of a contour stays below 2^53 units (GEOM_PERIM_UNITS_MAX) every partial sum of
// the sequential float64 loop is an integer count of 2^-23 below 2^53, hence exact, and the loop's result IS that total times 2^-23.
// A row whose total reaches the bound is refused by status (GEOM_ST_PERIMETER) and summed by the sequential host loop.  A call of more
// than GEOM_MAX_POINTS points is refused outright: below it no 64-bit total can wrap (2^23 segments of less than 2^40 units each).
//
// Hull capacity (a reasoned choice, not a measured one).  One wave keeps a contour's hull candidates - the points not strictly inside
// the octagon of its eight extreme points - in LDS, sorts them there and runs the monotone chain over them.  GEOM_HULL_CAP candidates
// are two 4 KiB arrays per wave.  A convex lattice polygon inside the coordinate bound can have a few thousand vertices (about
// 3.4 * 65536^(2/3) = 5500), contours of pixel blobs have tens and their candidates hundreds; 1024 covers those and keeps eight
// waves' worth of slots within 64 KiB of a compute unit's LDS.  A contour with more candidates gets GEOM_ST_HULL_CAP and is finished
// by the host routines: the result is the same.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VP_GEOM_HD __host__ __device__
#else
#define VP_GEOM_HD
#endif

#define GEOM_TB 64                      // threads of a block: one wave owns one contour (reasoned, not measured)
#define GEOM_HULL_CAP 1024              // hull candidates a wave keeps in LDS; a power of two (the sorting network's size)
#define GEOM_COORD_MIN (-32768)
#define GEOM_COORD_MAX 32767
#define GEOM_MAX_POINTS (1ll << 23)     // points of one call (of one frame of a batch)
#define GEOM_MAX_CONTOURS (1 << 24)     // contours of one call
#define GEOM_PERIM_UNITS_MAX (1ll << 53)
#define GEOM_UNIT 8388608.0             // 2^23

// status word of a row: 0 = finished on the device
#define GEOM_ST_OK 0u
#define GEOM_ST_HULL_CAP 1u             // more than GEOM_HULL_CAP hull candidates: hull, rectangle and circle not computed on the device
#define GEOM_ST_PERIMETER 2u            // the perimeter total reached 2^53 units: not the sequential sum
#define GEOM_ST_SKIPPED 4u              // batch form: the contour was not traced (beyond max_contours or max_points); the row is zero
#define GEOM_ST_COORD 8u                // device forms: a coordinate outside the bound; the row is zero

// What comes back from the device per contour: 64 bytes.  Points are (x, y) int16 pairs.
struct vp_geom_raw {
    int64_t perim_units;    // closed perimeter in units of 2^-23
    int64_t hull_area2;     // twice the hull's area
    float close_root;       // the closing segment (last point -> first point), for the open form
    int32_t hull_count;
    uint32_t status;        // GEOM_ST_* in bits 0..7, support points of the circle in bits 8..9
    int16_t edge[4];        // the winning hull edge of the calipers (hull_count == 1: the point, twice)
    int16_t ext[8];         // the hull vertices that gave amax, amin, bmax, bmin along / across that edge
    int16_t sup[6];         // support points of the enclosing circle
};

static inline const char* vp_geometry_refusal(long long n_contours, long long n_points, int* code)
{
    *code = -1;   // VP_ERR_INVALID
    if (n_contours < 0 || n_points < 0) return "contour geometry: negative count";
    *code = -4;   // VP_ERR_UNSUPPORTED
    if (n_contours > GEOM_MAX_CONTOURS) return "contour geometry: more than 2^24 contours in one call";
    if (n_points > GEOM_MAX_POINTS) return "contour geometry: more than 2^23 points; the 64-bit perimeter total (2^-23 units, exact below 2^53) could wrap";
    *code = 0;
    return NULL;
}

static inline size_t vp_geometry_align(size_t n) { return (n + 255) / 256 * 256; }
// what vp_contour_geometry_plan reports: an upper bound of the device bytes of a pass that starts from host points (upload of points,
// first indices and counts; rows; hull block when wanted).  The calls themselves declare their buffers on a vp_ws_frame.
static inline size_t vp_geometry_ws_bytes(long long n_contours, long long n_points, int hulls, int upload)
{
    size_t b = vp_geometry_align((size_t)n_contours * sizeof(vp_geom_raw)) + 4096;
    if (upload) b += vp_geometry_align((size_t)n_points * 8) + vp_geometry_align((size_t)n_contours * 8) + vp_geometry_align((size_t)n_contours * 4);
    if (hulls && upload) b += vp_geometry_align((size_t)n_points * 8);
    return b;
}

static inline bool vp_geometry_coord_ok(int32_t v) { return v >= GEOM_COORD_MIN && v <= GEOM_COORD_MAX; }

// ---- the arithmetic both sides share ----------------------------------------------------------------------------------------

// the float32 root of cv2_facade.arcLength for the segment (dx, dy), |dx|, |dy| < 2^17: products and sum rounded as float32 rounds
// them, the root through the double root (53 >= 2 * 24 + 2 bits: rounding it to float32 is the correctly rounded float32 root)
VP_GEOM_HD static inline float vp_geom_seg_root(int dx, int dy)
{
    const float fx = (float)dx, fy = (float)dy;
    const float xx = fx * fx, yy = fy * fy;
    const float s = xx + yy;
    return (float)sqrt((double)s);
}
VP_GEOM_HD static inline long long vp_geom_root_units(float root) { return (long long)((double)root * GEOM_UNIT); }

VP_GEOM_HD static inline uint32_t vp_geom_pack(int x, int y) { return ((uint32_t)(x + 32768) << 16) | (uint32_t)(y + 32768); }
VP_GEOM_HD static inline int vp_geom_px(uint32_t k) { return (int)(k >> 16) - 32768; }
VP_GEOM_HD static inline int vp_geom_py(uint32_t k) { return (int)(k & 0xffffu) - 32768; }

VP_GEOM_HD static inline long long vp_geom_cross(long long ox, long long oy, long long ax, long long ay, long long bx, long long by)
{
    return (ax - ox) * (by - oy) - (ay - oy) * (bx - ox);
}

// One hull edge of the calipers, in the doubles of vp_min_area_rect_i32: extents of the hull along (a) and across (b) the unit vector
// of edge i -> i + 1, scanned in vertex order; arg[] receives the first vertex that gave amax, amin, bmax, bmin.  hull: anything with
// x(k) and y(k) (the two views below).  Returns false for an edge of length 0.
struct vp_geom_hull_i32 { const int32_t* p; VP_GEOM_HD int x(int k) const { return p[2 * k]; } VP_GEOM_HD int y(int k) const { return p[2 * k + 1]; } };
struct vp_geom_hull_packed { const uint32_t* p; VP_GEOM_HD int x(int k) const { return vp_geom_px(p[k]); } VP_GEOM_HD int y(int k) const { return vp_geom_py(p[k]); } };
template <class H>
VP_GEOM_HD static inline bool vp_geom_edge_extents(const H& hull, int n, int i, double* ext4, int* arg4)
{
    const int i1 = (i + 1) % n;
    const double ex = (double)hull.x(i1) - (double)hull.x(i), ey = (double)hull.y(i1) - (double)hull.y(i);
    const double ln = sqrt(ex * ex + ey * ey);
    if (ln == 0) return false;
    const double ux = ex / ln, uy = ey / ln;
    double amax = 0, amin = 0, bmax = 0, bmin = 0;
    int ia = 0, ib = 0, ic = 0, id = 0;
    for (int k = 0; k < n; k++) {
        const double hx = (double)hull.x(k), hy = (double)hull.y(k);
        const double a = hx * ux + hy * uy, b = -hx * uy + hy * ux;
        if (k == 0) { amax = amin = a; bmax = bmin = b; }
        else {
            if (amax < a) { amax = a; ia = k; }
            if (a < amin) { amin = a; ib = k; }
            if (bmax < b) { bmax = b; ic = k; }
            if (b < bmin) { bmin = b; id = k; }
        }
    }
    ext4[0] = amax; ext4[1] = amin; ext4[2] = bmax; ext4[3] = bmin;
    arg4[0] = ia; arg4[1] = ib; arg4[2] = ic; arg4[3] = id;
    return true;
}

// ---- enclosing circle: exact containment in the circle a support set defines ---------------------------------------------------
// one point: equality; two: the circle on the diameter a b, (p - a).(p - b) <= 0; three: the in-circle determinant with the sign of the
// triangle's orientation (128-bit: entries below 2^17, 2^17 and 2^34).  true: p lies OUTSIDE.
struct vp_geom_support { int n; int x[3], y[3]; };

VP_GEOM_HD static inline bool vp_geom_outside(const vp_geom_support& s, int px, int py)
{
    if (s.n <= 0) return true;
    if (s.n == 1) return px != s.x[0] || py != s.y[0];
    if (s.n == 2) {
        const long long d = (long long)(px - s.x[0]) * (px - s.x[1]) + (long long)(py - s.y[0]) * (py - s.y[1]);
        return d > 0;
    }
    const long long adx = s.x[0] - px, ady = s.y[0] - py, bdx = s.x[1] - px, bdy = s.y[1] - py, cdx = s.x[2] - px, cdy = s.y[2] - py;
    const long long ad2 = adx * adx + ady * ady, bd2 = bdx * bdx + bdy * bdy, cd2 = cdx * cdx + cdy * cdy;
    const __int128 det = (__int128)adx * (bdy * cd2 - bd2 * cdy) - (__int128)ady * (bdx * cd2 - bd2 * cdx) + (__int128)ad2 * (bdx * cdy - bdy * cdx);
    const long long orient = vp_geom_cross(s.x[0], s.y[0], s.x[1], s.y[1], s.x[2], s.y[2]);
    // counter-clockwise a b c: det > 0 strictly inside, det < 0 outside
    return orient > 0 ? det < 0 : det > 0;
}

// The order the incremental algorithm visits n hull vertices in: t -> (t * stride) mod n with stride coprime to n and near 0.618 n, so
// that the first few vertices already span the hull (vertices in hull order, nearly cocircular for a disc, would make every vertex a
// new support point).  Deterministic; the circle does not depend on it.
VP_GEOM_HD static inline int vp_geom_stride(int n)
{
    if (n <= 2) return 1;
    int s = (int)(((long long)n * 618) / 1000);
    if (s < 1) s = 1;
    for (;; s++) {
        int a = n, b = s;
        while (b) { const int t = a % b; a = b; b = t; }
        if (a == 1) return s;
    }
}
