// Stereo rectification and 3-D reprojection: the head and the tail of the stereo stack.
//
// k_rectify_pair turns both eyes of a raw frame into what the matchers read, in one launch: per output pixel and eye the fixed
// bilinear gather of cv2.remap (vp_remap.hip's arithmetic with BORDER_CONSTANT 0) on every channel, rounded as the remap rounds, and
// from those rounded bytes cv2's grey.  The colour pixel is stored only where the caller keeps it; otherwise it lives in registers
// and the two colour intermediates of the composition (remap, then cvtColor) never reach HBM.  The eye is blockIdx.z, so every
// per-eye pointer is wave-uniform and comes from the kernel arguments by scalar loads.  The tile is the remap kernels': one lane owns
// RP_PPT adjacent pixels, its table loads are 16 + 8 bytes and its grey store 4 bytes wherever the row is whole groups and the
// pointers are aligned (the flags of rp_eye); ragged rows take scalar loads and byte stores.  No LDS: the maps of real lenses are
// smooth and the taps of neighbouring lanes share cache lines.  A tap is tested against the eye's own width and height before it is
// dereferenced, never against the stride: in a side-by-side frame the left eye's column w is the right eye's column 0.
//
// k_reproject is one pixel per thread: four rows of Q times (x, y, d, 1) in double and three double quotients (vp_rectify_plan.h has
// the operation order, shared with the host statement), 12 bytes stored per lane, adjacent lanes adjacent.
#include "vp_internal.h"
#include "vp_rectify_plan.h"

enum { RP_VEC_MAP = 1, RP_VEC_GREY = 2, RP_VEC_COLOUR = 4 };
struct rp_eye {
    const uint8_t* src; size_t sstride;
    const short* xy; const uint16_t* frac;
    uint8_t* grey; size_t gstride;
    uint8_t* colour; size_t cstride;      // colour == NULL: not kept
    int flags;                            // RP_VEC_*: which of this eye's accesses may be whole-group vector accesses
};
struct rp_args { rp_eye eye[2]; int w, h, ow, oh; };

template <int CN>
__global__ __launch_bounds__(64 * RP_TH) void k_rectify_pair(rp_args A)
{
    const rp_eye& E = A.eye[blockIdx.z];
    const int x0 = (int)(blockIdx.x * 64 + threadIdx.x) * RP_PPT, y = (int)(blockIdx.y * RP_TH + threadIdx.y);
    if (x0 >= A.ow || y >= A.oh) return;
    const int n = min(RP_PPT, A.ow - x0);
    const bool whole = n == RP_PPT;
    const size_t i0 = (size_t)y * A.ow + x0;
    int sx[RP_PPT], sy[RP_PPT], fr[RP_PPT];
    if (whole && (E.flags & RP_VEC_MAP)) {
        const uint4 q = *(const uint4*)(E.xy + 2 * i0);
        const uint2 f = *(const uint2*)(E.frac + i0);
        const u32 m[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < RP_PPT; i++) { sx[i] = (short)(m[i] & 0xffffu); sy[i] = (short)(m[i] >> 16); }
        fr[0] = f.x & 0xffffu; fr[1] = f.x >> 16; fr[2] = f.y & 0xffffu; fr[3] = f.y >> 16;
    } else {
#pragma unroll
        for (int i = 0; i < RP_PPT; i++) {
            const bool on = i < n;
            sx[i] = on ? E.xy[2 * (i0 + i)] : 0;
            sy[i] = on ? E.xy[2 * (i0 + i) + 1] : 0;
            fr[i] = on ? E.frac[i0 + i] : 0;
        }
    }
    uint8_t o[RP_PPT * CN], g[RP_PPT];
#pragma unroll
    for (int i = 0; i < RP_PPT; i++) {
        if (i < n) vp_rectify_sample<CN>(E.src, E.sstride, A.w, A.h, sx[i], sy[i], fr[i] & 1023, o + i * CN);
        else {
#pragma unroll
            for (int c = 0; c < CN; c++) o[i * CN + c] = 0;
        }
        g[i] = CN == 1 ? o[i] : (uint8_t)vp_rectify_grey(o[i * CN], o[i * CN + 1], o[i * CN + 2]);
    }
    uint8_t* gp = E.grey + (size_t)y * E.gstride + x0;
    if (whole && (E.flags & RP_VEC_GREY)) *(u32*)gp = (u32)g[0] | ((u32)g[1] << 8) | ((u32)g[2] << 16) | ((u32)g[3] << 24);
    else {
#pragma unroll
        for (int i = 0; i < RP_PPT; i++)
            if (i < n) gp[i] = g[i];
    }
    if (!E.colour) return;
    uint8_t* cp = E.colour + (size_t)y * E.cstride + (size_t)x0 * CN;
    if (whole && (E.flags & RP_VEC_COLOUR)) {
        u32 q[CN];
#pragma unroll
        for (int i = 0; i < CN; i++) q[i] = (u32)o[4 * i] | ((u32)o[4 * i + 1] << 8) | ((u32)o[4 * i + 2] << 16) | ((u32)o[4 * i + 3] << 24);
        if constexpr (CN == 4) *(uint4*)cp = make_uint4(q[0], q[1], q[2], q[3]);
        else {
#pragma unroll
            for (int i = 0; i < CN; i++) ((u32*)cp)[i] = q[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < RP_PPT * CN; i++)
            if (i < n * CN) cp[i] = o[i];
    }
}

static bool rp_aligned(const void* p, size_t stride, size_t a) { return (((uintptr_t)p | stride) & (a - 1)) == 0; }

// both eyes in one launch; every argument has been checked by the caller (vp_api_rectify.hip)
int vpk_rectify_pair(vp_ctx* ctx, const uint8_t* const* d_src, const size_t* sstride, int w, int h, int cn, const int16_t* const* d_xy, const uint16_t* const* d_frac,
                     int ow, int oh, uint8_t* const* d_grey, const size_t* gstride, uint8_t* const* d_colour, const size_t* cstride)
{
    rp_args A;
    A.w = w; A.h = h; A.ow = ow; A.oh = oh;
    for (int e = 0; e < 2; e++) {
        rp_eye& E = A.eye[e];
        E.src = d_src[e]; E.sstride = sstride[e];
        E.xy = (const short*)d_xy[e]; E.frac = d_frac[e];
        E.grey = d_grey[e]; E.gstride = gstride[e];
        E.colour = d_colour[e]; E.cstride = d_colour[e] ? cstride[e] : 0;
        E.flags = 0;
        if (ow % RP_PPT == 0 && rp_aligned(d_xy[e], 0, 16) && rp_aligned(d_frac[e], 0, 8)) E.flags |= RP_VEC_MAP;
        if (rp_aligned(d_grey[e], gstride[e], 4)) E.flags |= RP_VEC_GREY;
        if (d_colour[e] && rp_aligned(d_colour[e], cstride[e], cn == 4 ? 16 : 4)) E.flags |= RP_VEC_COLOUR;
    }
    const dim3 grid(vp_rectify_grid_x(ow), vp_rectify_grid_y(oh), 2), blk(64, RP_TH);
    vp_prof_scope ps(ctx, VPK_OTHER);
    if (cn == 1) hipLaunchKernelGGL(k_rectify_pair<1>, grid, blk, 0, ctx->stream, A);
    else if (cn == 3) hipLaunchKernelGGL(k_rectify_pair<3>, grid, blk, 0, ctx->stream, A);
    else hipLaunchKernelGGL(k_rectify_pair<4>, grid, blk, 0, ctx->stream, A);
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

struct rj_q { double q[16]; };

template <int TYPE>
__global__ __launch_bounds__(RJ_BLOCK) void k_reproject(const uint8_t* __restrict__ disp, size_t dstride, int w, rj_q Q, int invalid, float* __restrict__ xyz, size_t xpitch)
{
    const int x = blockIdx.x * RJ_BLOCK + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    float o[3];
    if (TYPE == VP_RJ_I16) vp_reproject_i16(Q.q, x, y, ((const int16_t*)(disp + (size_t)y * dstride))[x], invalid, o);
    else vp_reproject_f32(Q.q, x, y, ((const float*)(disp + (size_t)y * dstride))[x], o);
    float* p = xyz + (size_t)y * xpitch + (size_t)x * 3;
    p[0] = o[0]; p[1] = o[1]; p[2] = o[2];
}

int vpk_reproject(vp_ctx* ctx, const void* d_disp, size_t dstride, int disp_type, int w, int h, const double* q16, int invalid, float* d_xyz, size_t xstride)
{
    rj_q Q;
    for (int i = 0; i < 16; i++) Q.q[i] = q16[i];
    const dim3 grid((unsigned)((w + RJ_BLOCK - 1) / RJ_BLOCK), (unsigned)h);
    vp_prof_scope ps(ctx, VPK_OTHER);
    if (disp_type == VP_RJ_I16) hipLaunchKernelGGL(k_reproject<VP_RJ_I16>, grid, dim3(RJ_BLOCK), 0, ctx->stream, (const uint8_t*)d_disp, dstride, w, Q, invalid, d_xyz, xstride / 4);
    else hipLaunchKernelGGL(k_reproject<VP_RJ_F32>, grid, dim3(RJ_BLOCK), 0, ctx->stream, (const uint8_t*)d_disp, dstride, w, Q, invalid, d_xyz, xstride / 4);
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
