// Host arithmetic of the speckle filter and of the surface normals (vp_speckle.hip): the argument checks, the tile geometry of the
// region labelling with its workspace, and the one formula of a normal that the kernel and the host routine share.  Plain C++ - no HIP
// types, no kernels - and a pure function of its arguments, like vp_stereo_plan.h.  DESIGN.md section 4.35; tests/speckle_restate.py
// and tests/normals_restate.py are the statements.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define SP_MAX_SIDE 4096
#define SP_TILE 32               // a block labels a square tile of this side in LDS (a reasoned choice, not varied: DESIGN.md 4.35)
#define SP_THREADS 256           // four pixels of a row per thread: SP_TILE / 4 threads per row
#define SP_QUAD 4
#define SP_MAX_DIFF 65535        // the largest distance of two int16 values

static_assert(SP_TILE % SP_QUAD == 0 && SP_TILE * SP_TILE == SP_THREADS * SP_QUAD, "speckle: a thread owns one quad of the tile");
static_assert((long long)SP_MAX_SIDE * SP_MAX_SIDE < (1ll << 31), "speckle: a pixel index and a region's count fit int32");

#ifdef __HIPCC__
#define VP_SPECKLE_HD __host__ __device__
#else
#define VP_SPECKLE_HD
#endif

struct vp_speckle_plan {
    int tile;                      // side of a tile
    unsigned grid_x, grid_y;       // tiles
    int lpitch;                    // entries of a row of the label and the count image: w rounded up to a quad
    size_t lds_bytes;              // static LDS of the tile kernel: labels, values, counts
    size_t off_count, ws_bytes;    // the label image is at 0, the count image at off_count
};

static inline const char* vp_speckle_geometry_refusal(int w, int h)
{
    if (w < 1 || h < 1) return "filter_speckles: width and height must be at least 1";
    if (w > SP_MAX_SIDE || h > SP_MAX_SIDE) return "filter_speckles: width and height must be at most 4096";
    return nullptr;
}

// strides in bytes; new_val is what the caller passed (any int that is an int16 value)
static inline const char* vp_speckle_refusal(int w, int h, size_t sstride, size_t dstride, int new_val, int max_speckle_size, int max_diff)
{
    if (const char* why = vp_speckle_geometry_refusal(w, h)) return why;
    if (sstride < (size_t)w * 2 || dstride < (size_t)w * 2) return "filter_speckles: an image's stride is below the row";
    if (sstride % 2 || dstride % 2) return "filter_speckles: an image's stride is not a multiple of the element size";
    if (new_val < -32768 || new_val > 32767) return "filter_speckles: new_val must be an int16 value";
    if (max_speckle_size < 0 || (long long)max_speckle_size > (long long)w * h) return "filter_speckles: max_speckle_size must lie in 0..w*h";
    if (max_diff < 0 || max_diff > SP_MAX_DIFF) return "filter_speckles: max_diff must lie in 0..65535";
    return nullptr;
}

static inline size_t vp_speckle_align(size_t n) { return (n + 255) / 256 * 256; }

// arguments as vp_speckle_geometry_refusal admitted them
static inline void vp_speckle_make_plan(int w, int h, vp_speckle_plan* P)
{
    P->tile = SP_TILE;
    P->grid_x = (unsigned)((w + SP_TILE - 1) / SP_TILE);
    P->grid_y = (unsigned)((h + SP_TILE - 1) / SP_TILE);
    P->lpitch = (w + SP_QUAD - 1) / SP_QUAD * SP_QUAD;
    P->lds_bytes = (size_t)SP_TILE * SP_TILE * 3 * 4;
    P->off_count = vp_speckle_align((size_t)P->lpitch * h * 4);
    P->ws_bytes = 2 * P->off_count;
}

// two pixels that are 4-neighbours, neither equal to new_val, belong to one region
VP_SPECKLE_HD static inline bool vp_speckle_linked(int a, int b, int max_diff) { return (a > b ? a - b : b - a) <= max_diff; }

// ---- surface normals -------------------------------------------------------------------------------------------------------------
static inline const char* vp_normals_refusal(int w, int h, size_t zstride, size_t nstride, double focal_px, double cx, double cy, double max_jump_m)
{
    if (w < 1 || h < 1) return "normals: width and height must be at least 1";
    if (w > SP_MAX_SIDE || h > SP_MAX_SIDE) return "normals: width and height must be at most 4096";
    if (zstride < (size_t)w * 4) return "normals: the depth's stride is below the row";
    if (nstride < (size_t)w * 12) return "normals: the result's stride is below the row";
    if (zstride % 4 || nstride % 4) return "normals: an image's stride is not a multiple of the element size";
    if (!isfinite(focal_px) || !(focal_px > 0)) return "normals: focal_px must be finite and positive";
    if (!isfinite(cx) || !isfinite(cy)) return "normals: the principal point cx, cy must be finite";
    if (isnan(max_jump_m)) return "normals: max_jump_m is not a number";
    return nullptr;
}

// <= 0 or infinite: no guard, passed on as a negative bound
static inline double vp_normals_jump(double max_jump_m) { return (max_jump_m > 0 && isfinite(max_jump_m)) ? max_jump_m : -1.0; }

VP_SPECKLE_HD static inline bool vp_normals_usable(float z) { return z > 0.0f && z <= 3.402823466e+38f; }   // finite and positive (NaN fails both)

VP_SPECKLE_HD static inline double vp_normals_sqrt(double v)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __dsqrt_rn(v);
#else
    return sqrt(v);
#endif
}

// The normal at (x, y) from the centre's depth zc and its four neighbours' (all inside the image: the caller saw to that): every
// product, sum, quotient and the root rounded on its own in IEEE double, in the order of tests/normals_restate.py.  jump < 0: no guard.
// false: no normal.
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
VP_SPECKLE_HD static inline bool vp_normal_at(int x, int y, float zc, float zl, float zr, float zu, float zd, double f, double cx, double cy, double jump, float n[3])
{
    if (!(vp_normals_usable(zc) && vp_normals_usable(zl) && vp_normals_usable(zr) && vp_normals_usable(zu) && vp_normals_usable(zd))) return false;
    const double Zc = zc, Zl = zl, Zr = zr, Zu = zu, Zd = zd;
    if (jump >= 0) {
        if (!(fabs(Zl - Zc) <= jump && fabs(Zr - Zc) <= jump && fabs(Zu - Zc) <= jump && fabs(Zd - Zc) <= jump)) return false;
    }
    const double xm = (double)(x - 1) - cx, xc = (double)x - cx, xp = (double)(x + 1) - cx;
    const double ym = (double)(y - 1) - cy, yc = (double)y - cy, yp = (double)(y + 1) - cy;
    // du = P(x + 1, y) - P(x - 1, y), dv = P(x, y + 1) - P(x, y - 1), P = ((x - cx) Z / f, (y - cy) Z / f, Z)
    const double du0 = xp * Zr / f - xm * Zl / f, du1 = yc * Zr / f - yc * Zl / f, du2 = Zr - Zl;
    const double dv0 = xc * Zd / f - xc * Zu / f, dv1 = yp * Zd / f - ym * Zu / f, dv2 = Zd - Zu;
    // c = dv x du: towards the camera
    const double c0 = dv1 * du2 - dv2 * du1, c1 = dv2 * du0 - dv0 * du2, c2 = dv0 * du1 - dv1 * du0;
    const double len = vp_normals_sqrt((c0 * c0 + c1 * c1) + c2 * c2);
    if (!(len > 0 && len <= 1.7976931348623157e308)) return false;   // zero; or, after an overflow on the way, infinite or not a number
    n[0] = (float)(c0 / len);
    n[1] = (float)(c1 / len);
    n[2] = (float)(c2 / len);
    return true;
}

// the three floats written for a pixel: the normal, or without one NaN (0x7fc00000); encoded: (n + 1) / 2 in float32, 0 without one
VP_SPECKLE_HD static inline void vp_normal_store(bool have, const float n[3], int encode, float* out)
{
    for (int i = 0; i < 3; i++) {
        if (encode) out[i] = have ? (float)((float)(n[i] + 1.0f) / 2.0f) : 0.0f;
        else if (have) out[i] = n[i];
        else {
            const uint32_t q = 0x7fc00000u;
            memcpy(&out[i], &q, 4);
        }
    }
}
