// Tile constants, refusals and the shared formulas of stereo rectification and 3-D reprojection (vp_rectify.hip, vp_api_rectify.hip).
// Plain C++ - no HIP types, no kernels - and pure functions of their arguments, like vp_remap_plan.h; the formulas are compiled for
// the device and for the host from this one text, so the _host entries state what the kernels compute.
#pragma once
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define VP_RECTIFY_HD __host__ __device__
#else
#define VP_RECTIFY_HD
#endif

// the tile of k_rectify_pair: one wave per destination row, RP_PPT adjacent pixels per lane (vp_remap.hip's shape, not varied here)
#define RP_PPT 4           // destination pixels per lane: 16 bytes of int16 x,y table, 8 of fractions, 4 grey bytes stored at once
#define RP_TW 256          // destination pixels per tile row: 64 lanes x RP_PPT
#define RP_TH 4            // destination rows per tile (256 threads)
#define RP_MAX_SIDE 4096   // source and destination, as the matchers that read the result
#define RJ_BLOCK 256       // k_reproject: one pixel per thread, one row per blockIdx.y
#define RJ_MAX_Q 1e100     // |Q entries|: keeps every sum finite, so no NaN arises whose sign would differ between host and device

// BGR -> grey of cv2 (Q14): what vp_cvt_color's BGR2GRAY / BGRA2GRAY computes
VP_RECTIFY_HD static inline int vp_rectify_grey(int b, int g, int r) { return (b * 1868 + g * 9617 + r * 4899 + 8192) >> 14; }

// One output pixel of one eye: the fixed bilinear gather of cv2.remap (INTER_LINEAR, BORDER_CONSTANT 0) at the integer part (sx, sy)
// and fraction index frac (fy * 32 + fx) into o[0..cn).  A tap outside [0, w) x [0, h) of this eye is 0 and is never dereferenced.
template <int CN>
VP_RECTIFY_HD static inline void vp_rectify_sample(const uint8_t* src, size_t stride, int w, int h, int sx, int sy, int frac, uint8_t* o)
{
    const int fx = frac & 31, fy = (frac >> 5) & 31;
    const int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32, w10 = (32 - fx) * fy * 32, w11 = fx * fy * 32;
    const bool x0in = sx >= 0 && sx < w, x1in = sx + 1 >= 0 && sx + 1 < w, y0in = sy >= 0 && sy < h, y1in = sy + 1 >= 0 && sy + 1 < h;
    const uint8_t* r0 = src + (size_t)(y0in ? sy : 0) * stride;
    const uint8_t* r1 = src + (size_t)(y1in ? sy + 1 : 0) * stride;
    const size_t c0 = (size_t)(x0in ? sx : 0) * CN, c1 = (size_t)(x1in ? sx + 1 : 0) * CN;
#pragma unroll
    for (int c = 0; c < CN; c++) {
        const int v00 = (x0in && y0in) ? r0[c0 + c] : 0, v01 = (x1in && y0in) ? r0[c1 + c] : 0;
        const int v10 = (x0in && y1in) ? r1[c0 + c] : 0, v11 = (x1in && y1in) ? r1[c1 + c] : 0;
        o[c] = (uint8_t)((v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11 + (1 << 14)) >> 15);   // the weights sum to 2^15: at most 255
    }
}

// launch geometry: blocks of (64, RP_TH) threads, the eye is blockIdx.z
static inline unsigned vp_rectify_grid_x(int out_w) { return (unsigned)((out_w + RP_TW - 1) / RP_TW); }
static inline unsigned vp_rectify_grid_y(int out_h) { return (unsigned)((out_h + RP_TH - 1) / RP_TH); }

static inline const char* vp_rectify_size_refusal(int w, int h, int cn, int out_w, int out_h)
{
    if (w < 1 || h < 1 || out_w < 1 || out_h < 1) return "rectify: widths and heights must be at least 1";
    if (w > RP_MAX_SIDE || h > RP_MAX_SIDE || out_w > RP_MAX_SIDE || out_h > RP_MAX_SIDE) return "rectify: widths and heights must be at most 4096";
    if (cn != 1 && cn != 3 && cn != 4) return "rectify: cn must be 1, 3 (BGR) or 4 (BGRA)";
    return nullptr;
}

// ---- reprojection -------------------------------------------------------------------------------------------------------------------
#define VP_RJ_I16 0        // VP_DISP_I16 / VP_DISP_F32 of include/vp.h
#define VP_RJ_F32 1

// (X, Y, Z, W) = Q (x, y, d, 1) in double, every row ((q0 x + q1 y) + q2 d) + q3 with one rounding per product and sum (the library
// is built with -ffp-contract=off; the pragma keeps that true for this text wherever it is compiled), then X / W, Y / W, Z / W, each
// one double quotient rounded once more to float32.  W == 0 gives three zeros.
VP_RECTIFY_HD static inline void vp_reproject_point(const double* q, double x, double y, double d, float* o)
{
#pragma clang fp contract(off)
    const double X = ((q[0] * x + q[1] * y) + q[2] * d) + q[3];
    const double Y = ((q[4] * x + q[5] * y) + q[6] * d) + q[7];
    const double Z = ((q[8] * x + q[9] * y) + q[10] * d) + q[11];
    const double W = ((q[12] * x + q[13] * y) + q[14] * d) + q[15];
    if (W == 0.0) { o[0] = o[1] = o[2] = 0.0f; return; }
    o[0] = (float)(X / W);
    o[1] = (float)(Y / W);
    o[2] = (float)(Z / W);
}

// a pixel of the disparity image -> its three floats; int16 disparities are sixteenths of a pixel (d / 16 is exact in double)
VP_RECTIFY_HD static inline void vp_reproject_i16(const double* q, int x, int y, int d16, int invalid, float* o)
{
    if (d16 == invalid) { o[0] = o[1] = o[2] = 0.0f; return; }
    vp_reproject_point(q, (double)x, (double)y, (double)d16 / 16.0, o);
}
VP_RECTIFY_HD static inline void vp_reproject_f32(const double* q, int x, int y, float d, float* o)
{
    if (!(d - d == 0.0f)) { o[0] = o[1] = o[2] = 0.0f; return; }      // NaN and the infinities
    vp_reproject_point(q, (double)x, (double)y, (double)d, o);
}

static inline const char* vp_reproject_refusal(int disp_type, int w, int h, size_t disp_stride, const double* q16, int invalid_disp, size_t xyz_stride)
{
    if (disp_type != VP_RJ_I16 && disp_type != VP_RJ_F32) return "reproject: disp_type must be VP_DISP_I16 or VP_DISP_F32";
    const size_t es = disp_type == VP_RJ_I16 ? 2 : 4;
    if (w < 1 || h < 1) return "reproject: width and height must be at least 1";
    if (w > RP_MAX_SIDE || h > RP_MAX_SIDE) return "reproject: width and height must be at most 4096";
    if (disp_stride < (size_t)w * es) return "reproject: the disparity's stride is below the row";
    if (disp_stride % es) return "reproject: the disparity's stride is not a multiple of the element size";
    if (xyz_stride < (size_t)w * 12) return "reproject: the result's stride is below the row";
    if (xyz_stride % 4) return "reproject: the result's stride is not a multiple of 4";
    if (!q16) return "reproject: Q is missing";
    for (int i = 0; i < 16; i++)
        if (!(std::fabs(q16[i]) <= RJ_MAX_Q)) return "reproject: Q must be finite, its entries at most 1e100 in magnitude";
    if (invalid_disp != INT_MIN && (disp_type != VP_RJ_I16 || invalid_disp < -32768 || invalid_disp > 32767))
        return "reproject: invalid_disp must be INT_MIN (none) or an int16 value of an int16 disparity image";
    return nullptr;
}
