// Filled shapes in a packed device image (vp_fill_polys_dev, vp_fill_rect_dev, vp_fill_circle_dev): the even-odd scanline of
// vision/utils/draw.py _fill, the numpy slices of draw_rect / draw_circle.  Every kernel here is "one wave per image row": the wave
// finds the row's spans and writes each with 16-byte stores between two ragged ends.
#include "vp_internal.h"
#include "vp_fill_span.h"
#include <algorithm>

// One wave (= one block) per row of one polygon.  The lanes stride over the polygon's edges; those that meet the row put their
// crossing key into LDS at the place a ballot prefix gives them; the keys are sorted by rank (each lane counts the keys in front of
// its own: rows have a handful of crossings, at most VP_FILL_MAX_CROSS); pair i of the sorted list is the span ceil(k[2i]) ..
// floor(k[2i+1]).
__device__ __forceinline__ void fill_poly_row(uint8_t* __restrict__ img, int w, int cn, const int2* __restrict__ pts, const vp_fill_poly* __restrict__ polys, int npolys,
                                              int row, u32 cw, u64* keys, u64* sorted)
{
    const int lane = threadIdx.x;
    int lo = 0, hi = npolys - 1;                          // the last polygon whose row_base <= row
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (polys[mid].row_base <= row) lo = mid; else hi = mid - 1;
    }
    const vp_fill_poly P = polys[lo];
    const int y = P.y0 + (row - P.row_base);
    if (row - P.row_base >= P.rows) return;
    int total = 0;
    for (int base = 0; base < P.count; base += 64) {
        const int i = base + lane;
        bool hit = false;
        u64 key = 0;
        if (i < P.count) {
            const int2 a = pts[P.first + i], b = pts[P.first + (i + 1 == P.count ? 0 : i + 1)];
            if (vp_fill_edge_on_row(a.y, b.y, y)) {
                hit = true;
                key = vp_fill_cross_key(a.x, a.y, b.x, b.y, y);
            }
        }
        const u64 m = __ballot(hit);
        if (hit) {
            const int at = total + __popcll(m & ((1ull << lane) - 1ull));
            if (at < VP_FILL_MAX_CROSS) keys[at] = key;
        }
        total += __popcll(m);
    }
    if (total > VP_FILL_MAX_CROSS) return;                // not reached: vp_fill_polys_dev has counted every row's crossings by the same vp_fill_edge_rows
    __syncthreads();
    for (int i = lane; i < total; i += 64) {
        const u64 key = keys[i];
        int rank = 0;
        for (int j = 0; j < total; j++) {
            const u64 kj = keys[j];
            rank += (kj < key || (kj == key && j < i)) ? 1 : 0;
        }
        sorted[rank] = key;
    }
    __syncthreads();
    for (int i = 0; i + 1 < total; i += 2)
        fill_columns(img, w, cn, y, vp_fill_key_ceil(sorted[i]), vp_fill_key_floor(sorted[i + 1]), cw, lane);
}

__global__ __launch_bounds__(64) void k_fill_polys(uint8_t* __restrict__ img, int w, int cn, const int2* __restrict__ pts, const vp_fill_poly* __restrict__ polys,
                                                   int npolys, int total_rows, u32 cw)
{
    __shared__ u64 keys[VP_FILL_MAX_CROSS], sorted[VP_FILL_MAX_CROSS];
    if ((int)blockIdx.x >= total_rows) return;
    fill_poly_row(img, w, cn, pts, polys, npolys, (int)blockIdx.x, cw, keys, sorted);
}

// a few vertices travel as kernel arguments, as the outline's do (k_draw_small)
#define VP_FILL_SMALL_PTS 48
struct fill_small { int2 pts[VP_FILL_SMALL_PTS]; vp_fill_poly polys[VP_FILL_SMALL_POLYS]; };
__global__ __launch_bounds__(64) void k_fill_polys_small(uint8_t* __restrict__ img, int w, int cn, fill_small S, int npolys, int total_rows, u32 cw)
{
    __shared__ u64 keys[VP_FILL_MAX_CROSS], sorted[VP_FILL_MAX_CROSS];
    if ((int)blockIdx.x >= total_rows) return;
    fill_poly_row(img, w, cn, S.pts, S.polys, npolys, (int)blockIdx.x, cw, keys, sorted);
}

__global__ __launch_bounds__(64) void k_fill_rect(uint8_t* __restrict__ img, int w, int cn, int xa, int xb, int ya, int yb, u32 cw)
{
    const int y = ya + (int)blockIdx.x;
    if (y > yb) return;
    fill_columns(img, w, cn, y, xa, xb, cw, threadIdx.x);
}

// rows y0 .. y1 (already clipped to the image) of the disc
__global__ __launch_bounds__(64) void k_fill_disc(uint8_t* __restrict__ img, int w, int cn, int cx, int cy, int r, int y0, int y1, u32 cw)
{
    const int y = y0 + (int)blockIdx.x;
    if (y > y1) return;
    const long long dy = (long long)y - cy, v = (long long)r * r - dy * dy;
    if (v < 0) return;
    long long s = (long long)sqrt((double)v);             // v < 2^41: the estimate is off by one at most, the two loops make it exact
    while (s * s > v) s--;
    while ((s + 1) * (s + 1) <= v) s++;
    fill_columns(img, w, cn, y, (long long)cx - s, (long long)cx + s, cw, threadIdx.x);
}

static u32 color_word(const uint8_t* color, int cn)
{
    u32 cw = 0;
    for (int c = 0; c < cn; c++) cw |= (u32)color[c] << (8 * c);
    return cw;
}

int vpk_fill_polys(vp_ctx* ctx, uint8_t* d_img, int w, int h, int cn, const int32_t* pts, int npts, const vp_fill_poly* polys, int npolys, int total_rows,
                   const uint8_t* color, bool on_host)
{
    (void)h;
    if (npolys <= 0 || total_rows <= 0) return VP_OK;
    const u32 cw = color_word(color, cn);
    if (on_host) {
        if (npts > VP_FILL_SMALL_PTS || npolys > VP_FILL_SMALL_POLYS) return vp_fail(ctx, VP_ERR_INVALID, "vpk_fill_polys: too many points for the argument form");
        fill_small S;
        for (int i = 0; i < npts; i++) S.pts[i] = make_int2(pts[2 * i], pts[2 * i + 1]);
        for (int i = npts; i < VP_FILL_SMALL_PTS; i++) S.pts[i] = make_int2(0, 0);
        for (int i = 0; i < VP_FILL_SMALL_POLYS; i++) S.polys[i] = polys[i < npolys ? i : npolys - 1];
        hipLaunchKernelGGL(k_fill_polys_small, dim3((unsigned)total_rows), dim3(64), 0, ctx->stream, d_img, w, cn, S, npolys, total_rows, cw);
    } else {
        hipLaunchKernelGGL(k_fill_polys, dim3((unsigned)total_rows), dim3(64), 0, ctx->stream, d_img, w, cn, reinterpret_cast<const int2*>(pts), polys, npolys,
                           total_rows, cw);
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

int vpk_fill_rect(vp_ctx* ctx, uint8_t* d_img, int w, int h, int cn, int xa, int xb, int ya, int yb, const uint8_t* color)
{
    if (xa < 0 || ya < 0 || xb >= w || yb >= h || xa > xb || ya > yb) return vp_fail(ctx, VP_ERR_INVALID, "vpk_fill_rect: not clipped");
    hipLaunchKernelGGL(k_fill_rect, dim3((unsigned)(yb - ya + 1)), dim3(64), 0, ctx->stream, d_img, w, cn, xa, xb, ya, yb, color_word(color, cn));
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

int vpk_fill_disc(vp_ctx* ctx, uint8_t* d_img, int w, int h, int cn, int cx, int cy, int r, const uint8_t* color)
{
    const long long y0 = std::max<long long>((long long)cy - r, 0), y1 = std::min<long long>((long long)cy + r, h - 1);
    if (r < 0 || y0 > y1) return VP_OK;
    hipLaunchKernelGGL(k_fill_disc, dim3((unsigned)(y1 - y0 + 1)), dim3(64), 0, ctx->stream, d_img, w, cn, cx, cy, r, (int)y0, (int)y1, color_word(color, cn));
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
