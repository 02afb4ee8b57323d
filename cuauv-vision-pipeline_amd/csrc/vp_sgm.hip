// Semi-global stereo matching (tests/sgm_restate.py is the statement; geometry and workspace: vp_sgm_plan.h).
// The prefilter is the block matcher's launch (vpk_stereo_prefilter), which also writes the invalid value into every pixel of the result.
//   k_sgm_cost    the window SAD of the prefiltered images as uint16 C[y][x][d] over the candidate rectangle, d fastest.  A block makes
//                 one candidate row of SG_STRIP columns: the window's rows staged in LDS, vertical sums per column and disparity (two
//                 disparities to a 32-bit word), then the sum of 2 r + 1 columns; one 32-bit store per lane, contiguous over the wave.
//   k_sgm_path    one direction of travel.  `group` lanes hold the disparities of one pixel of one line, K consecutive ones each, and
//                 walk the line: L(q, .) stays in registers, the d -+ 1 neighbours of a lane's first and last disparity come from the
//                 lanes beside it, min over k of L(q, k) by a butterfly over the group.  A wave holds 64 / group lines; lines never wait
//                 on one another, so the grid is the set of lines.  The first direction writes S, the others add to it: launches
//                 queued on one stream, plain read-modify-write, an exact integer sum.
//   k_sgm_select  per pixel, in the same lane layout: the best disparity (ties to the larger), the uniqueness scan, the right view's
//                 answer along the diagonal of S, the subpixel step.
// Every index into C and S is a size_t: under the 4 GiB cap a volume holds up to 2^30 entries of two bytes (4096 x 1090 x 256 comes close),
// so byte offsets reach 2^31 and S lies further than that from the workspace's start.
#include "vp_internal.h"
#include "vp_sgm_plan.h"

int vpk_stereo_prefilter(vp_ctx* ctx, const uint8_t* d_left, size_t lstride, const uint8_t* d_right, size_t rstride, int w, int h, int cap, int min_disp, uint8_t* pl,
                         uint8_t* pr, size_t pitch, int16_t* d_disp, size_t dstride);

#define SG_BIG (1 << 29)     // a path cost that never wins; SG_BIG + p2 stays inside int

struct sg_cost_args {
    int w, nd, min_disp;
    vp_sgm_plan P;
};

__device__ __forceinline__ u32 sg_absdiff(int a, int b) { return (u32)(a > b ? a - b : b - a); }

__global__ __launch_bounds__(SG_COST_THREADS) void k_sgm_cost(const uint8_t* __restrict__ pl, const uint8_t* __restrict__ pr, sg_cost_args A, u32* __restrict__ C2)
{
    extern __shared__ __attribute__((aligned(16))) u32 sg_lds[];
    const vp_sgm_plan& P = A.P;
    const int t = threadIdx.x, r = P.r, nd = A.nd, ndp = P.ndp, ncols = P.ncols, nrcols = P.nrcols, rows = 2 * r + 1;
    u32* V = sg_lds + P.off_v;                                     // [ncols][ndp]: vertical sums of disparities 2 dp (low half) and 2 dp + 1
    uint8_t* lrow = (uint8_t*)(sg_lds + P.off_rows);               // [rows][lpitch]
    uint8_t* rrow = lrow + rows * P.lpitch;                        // [rows][rpitch]
    const int xs = P.cx0 + (int)blockIdx.x * SG_STRIP;             // the strip's first candidate column
    const int yc = (int)blockIdx.y, y = P.cy0 + yc;                // the candidate row: all rows y - r .. y + r lie inside the image
    const int px_end = min(SG_STRIP, P.cx0 + P.cw - xs);
    const int colbase = xs - r;                                    // image column of vertical-sum column 0
    const int rbase = colbase - (A.min_disp + nd - 1);             // image column of a staged right row's byte 0
    const size_t pitch = P.pitch;

    for (int i = t; i < rows * ncols; i += SG_COST_THREADS) {
        const int j = i / ncols, c = i - j * ncols, col = colbase + c;
        lrow[j * P.lpitch + c] = col >= 0 && col < A.w ? pl[(size_t)(y - r + j) * pitch + col] : (uint8_t)0;
    }
    for (int i = t; i < rows * nrcols; i += SG_COST_THREADS) {
        const int j = i / nrcols, c = i - j * nrcols, col = rbase + c;
        rrow[j * P.rpitch + c] = col >= 0 && col < A.w ? pr[(size_t)(y - r + j) * pitch + col] : (uint8_t)0;
    }
    __syncthreads();
    for (int i = t; i < ncols * ndp; i += SG_COST_THREADS) {
        const int c = i / ndp, dp = i - c * ndp, j = c + nd - 1 - 2 * dp;       // right byte of the even disparity; the odd one is at j - 1
        u32 acc = 0;
        for (int k = 0; k < rows; k++) {
            const int l = lrow[k * P.lpitch + c];
            acc += sg_absdiff(l, rrow[k * P.rpitch + j]) | (sg_absdiff(l, rrow[k * P.rpitch + j - 1]) << 16);
        }
        V[i] = acc;
    }
    __syncthreads();
    u32* out = C2 + ((size_t)yc * P.cw + (size_t)(xs - P.cx0)) * ndp;
    for (int i = t; i < px_end * ndp; i += SG_COST_THREADS) {
        const int x = i / ndp, dp = i - x * ndp;
        u32 acc = 0;
        for (int k = 0; k < rows; k++) acc += V[(x + k) * ndp + dp];             // no carry between the halves: a window sum is below 2^16
        out[i] = acc;
    }
}

// K consecutive uint16 entries at p (aligned to 2 K bytes: d0 is a multiple of K and every pixel's row of C and S starts on 32 bytes)
template <int K> __device__ __forceinline__ void sg_load(const uint16_t* p, int (&v)[K]);
template <> __device__ __forceinline__ void sg_load<1>(const uint16_t* p, int (&v)[1]) { v[0] = *p; }
template <> __device__ __forceinline__ void sg_load<2>(const uint16_t* p, int (&v)[2])
{
    const u32 a = *(const u32*)p;
    v[0] = (int)(a & 0xffffu);
    v[1] = (int)(a >> 16);
}
template <> __device__ __forceinline__ void sg_load<4>(const uint16_t* p, int (&v)[4])
{
    const uint2 a = *(const uint2*)p;
    v[0] = (int)(a.x & 0xffffu);
    v[1] = (int)(a.x >> 16);
    v[2] = (int)(a.y & 0xffffu);
    v[3] = (int)(a.y >> 16);
}
template <int K> __device__ __forceinline__ void sg_store(uint16_t* p, const int (&v)[K]);
template <> __device__ __forceinline__ void sg_store<1>(uint16_t* p, const int (&v)[1]) { *p = (uint16_t)v[0]; }
template <> __device__ __forceinline__ void sg_store<2>(uint16_t* p, const int (&v)[2]) { *(u32*)p = (u32)v[0] | ((u32)v[1] << 16); }
template <> __device__ __forceinline__ void sg_store<4>(uint16_t* p, const int (&v)[4]) { *(uint2*)p = make_uint2((u32)v[0] | ((u32)v[1] << 16), (u32)v[2] | ((u32)v[3] << 16)); }

template <int K>
__global__ __launch_bounds__(SG_AGG_THREADS) void k_sgm_path(const uint16_t* __restrict__ C, uint16_t* __restrict__ S, int cw, int ch, int nd, int group, int dy, int dx, int p1,
                                                             int p2, int first)
{
    const int lane = threadIdx.x, g = lane / group, dl = lane - g * group, d0 = dl * K;
    const int line = (int)blockIdx.x * (SG_WAVE / group) + g;
    int x = 0, y = 0, len = 0;
    if (line < vp_sgm_line_count(cw, ch, dy, dx)) vp_sgm_line(cw, ch, dy, dx, line, &x, &y, &len);
    const bool mine = d0 < nd;                                     // n is a multiple of 16 and of K: a lane's slots are all inside or all idle
    int steps = len;                                               // the wave walks as long as its longest line; every lane takes every shuffle
    for (int o = SG_WAVE / 2; o; o >>= 1) steps = max(steps, __shfl_xor(steps, o));
    const ptrdiff_t step = ((ptrdiff_t)dy * cw + dx) * nd;
    size_t e = ((size_t)y * cw + x) * nd + d0;
    int L[K], c[K], M = 0;
    for (int k = 0; k < K; k++) { L[k] = SG_BIG; c[k] = 0; }
    if (mine && len > 0) sg_load<K>(C + e, c);
    for (int t = 0; t < steps; t++) {
        const bool on = mine && t < len;
        int cn[K], s[K];
        for (int k = 0; k < K; k++) cn[k] = s[k] = 0;
        if (mine && t + 1 < len) sg_load<K>(C + (e + step), cn);   // the next pixel's costs, asked for before this pixel's chain
        if (on && !first) sg_load<K>(S + e, s);
        int up = __shfl_up(L[K - 1], 1, group), dn = __shfl_down(L[0], 1, group);
        if (dl == 0) up = SG_BIG;                                  // d - 1 < 0: the term is absent
        if (dl == group - 1) dn = SG_BIG;                          // d + 1 >= n: absent (a lane past n holds SG_BIG by itself)
        int Ln[K], m = SG_BIG;
        for (int k = 0; k < K; k++) {
            const int left = k ? L[k - 1] : up, right = k < K - 1 ? L[k + 1] : dn;
            const int best = min(min(L[k], M + p2), min(left, right) + p1);
            Ln[k] = !on ? SG_BIG : (t == 0 ? c[k] : c[k] + best - M);
            m = min(m, Ln[k]);
        }
        for (int o = group >> 1; o; o >>= 1) m = min(m, __shfl_xor(m, o));
        M = m;
        for (int k = 0; k < K; k++) {
            L[k] = Ln[k];
            s[k] += Ln[k];
            c[k] = cn[k];
        }
        if (on) sg_store<K>(S + e, s);
        e += step;
    }
}

template <int K>
__global__ __launch_bounds__(SG_SEL_THREADS) void k_sgm_select(const uint16_t* __restrict__ S, int cw, int ch, int cx0, int cy0, int nd, int group, int min_disp, int uniq,
                                                               int diff, int16_t* __restrict__ disp, size_t dstride)
{
    const int lane = threadIdx.x & (SG_WAVE - 1), wave = threadIdx.x / SG_WAVE, per_wave = SG_WAVE / group;
    const int g = lane / group, dl = lane - g * group, d0 = dl * K;
    const size_t px = (size_t)blockIdx.x * (SG_SEL_THREADS / group) + (size_t)(wave * per_wave + g), npx = (size_t)cw * ch;
    const bool valid = px < npx, mine = valid && d0 < nd;
    const int y = valid ? (int)(px / (size_t)cw) : 0, x = valid ? (int)(px - (size_t)y * cw) : 0;
    int s[K];
    for (int k = 0; k < K; k++) s[k] = 0;
    if (mine) sg_load<K>(S + px * nd + d0, s);
    // the smallest sum, ties to the larger disparity: the sum above 255 - d
    u32 key = 0xffffffffu;
    for (int k = 0; k < K; k++)
        if (mine) key = min(key, ((u32)s[k] << 8) | (u32)(255 - (d0 + k)));
    for (int o = group >> 1; o; o >>= 1) key = min(key, (u32)__shfl_xor((int)key, o));
    const int ds = 255 - (int)(key & 255u), smin = (int)(key >> 8);
    bool keep = true;
    if (uniq > 0) {                                                // (uniform) the best rival more than one disparity away
        u32 rival = 0xffffffffu;
        for (int k = 0; k < K; k++) {
            const int d = d0 + k;
            if (mine && (d < ds - 1 || d > ds + 1)) rival = min(rival, (u32)s[k]);
        }
        for (int o = group >> 1; o; o >>= 1) rival = min(rival, (u32)__shfl_xor((int)rival, o));
        keep = !(rival <= (u32)(smin + smin * uniq / 100));
    }
    if (diff >= 0) {                                               // (uniform) the right view's answer at column x - (m + ds): S along x' - d = x - ds
        u32 kr = 0xffffffffu;
        for (int k = 0; k < K; k++) {
            const int d = d0 + k, xc = x - ds + d;
            if (mine && xc >= 0 && xc < cw) kr = min(kr, ((u32)S[((size_t)y * cw + xc) * nd + d] << 8) | (u32)(255 - d));
        }
        for (int o = group >> 1; o; o >>= 1) kr = min(kr, (u32)__shfl_xor((int)kr, o));
        const int dr = 255 - (int)(kr & 255u);
        if ((dr > ds ? dr - ds : ds - dr) > diff) keep = false;
    }
    if (valid && dl == 0) {
        int16_t out = (int16_t)vp_stereo_invalid(min_disp);
        if (keep) {
            const int dm = ds > 0 ? ds - 1 : ds + 1, dq = ds < nd - 1 ? ds + 1 : ds - 1;
            out = vp_stereo_subpixel(smin, S[px * nd + dm], S[px * nd + dq], min_disp + ds);
        }
        disp[(size_t)(cy0 + y) * dstride + cx0 + x] = out;
    }
}

template <int K>
static void sg_launch_paths(vp_ctx* ctx, const vp_sgm_plan& P, const uint16_t* C, uint16_t* S, int nd, int p1, int p2, int paths)
{
    for (int i = 0; i < paths; i++) {
        const int dy = vp_sgm_dirs[i][0], dx = vp_sgm_dirs[i][1];
        const unsigned grid = dy == 0 ? P.agg_gh : (dx == 0 ? P.agg_gv : P.agg_gd);
        vp_prof_scope ps(ctx, VPK_SGM_PATH);
        hipLaunchKernelGGL(k_sgm_path<K>, dim3(grid), dim3(SG_AGG_THREADS), 0, ctx->stream, C, S, P.cw, P.ch, nd, P.group, dy, dx, p1, p2, i == 0 ? 1 : 0);
    }
}

template <int K>
static void sg_launch_select(vp_ctx* ctx, const vp_sgm_plan& P, const uint16_t* S, int nd, int min_disp, int uniq, int diff, int16_t* d_disp, size_t dstride)
{
    vp_prof_scope ps(ctx, VPK_SGM_SELECT);
    hipLaunchKernelGGL(k_sgm_select<K>, dim3(P.sel_g), dim3(SG_SEL_THREADS), 0, ctx->stream, S, P.cw, P.ch, P.cx0, P.cy0, nd, P.group, min_disp, uniq, diff, d_disp, dstride / 2);
}

int vpk_stereo_sgm(vp_ctx* ctx, const uint8_t* d_left, size_t lstride, const uint8_t* d_right, size_t rstride, int w, int h, int nd, int min_disp, int cap, int p1, int p2,
                   int uniq, int diff, int paths, const vp_sgm_plan& P, uint8_t* d_ws, int16_t* d_disp, size_t dstride)
{
    uint8_t *pl = d_ws, *pr = d_ws + P.off_right;
    uint16_t *C = (uint16_t*)(d_ws + P.off_c), *S = (uint16_t*)(d_ws + P.off_s);
    if (int rc = vpk_stereo_prefilter(ctx, d_left, lstride, d_right, rstride, w, h, cap, min_disp, pl, pr, P.pitch, d_disp, dstride)) return rc;
    if (!P.cw) return VP_OK;
    if (P.cost_lds > SB_LDS_BYTES) return vp_fail(ctx, VP_ERR_UNSUPPORTED, "sgm: the cost block's tables are above the LDS budget");
    sg_cost_args A = {w, nd, min_disp, P};
    {
        vp_prof_scope ps(ctx, VPK_SGM_COST);
        hipLaunchKernelGGL(k_sgm_cost, dim3(P.cost_gx, P.cost_gy), dim3(SG_COST_THREADS), P.cost_lds, ctx->stream, pl, pr, A, (u32*)C);
    }
    VP_HIP(ctx, hipGetLastError());
    switch (P.per_lane) {
    case 1: sg_launch_paths<1>(ctx, P, C, S, nd, p1, p2, paths); break;
    case 2: sg_launch_paths<2>(ctx, P, C, S, nd, p1, p2, paths); break;
    default: sg_launch_paths<4>(ctx, P, C, S, nd, p1, p2, paths); break;
    }
    VP_HIP(ctx, hipGetLastError());
    switch (P.per_lane) {
    case 1: sg_launch_select<1>(ctx, P, S, nd, min_disp, uniq, diff, d_disp, dstride); break;
    case 2: sg_launch_select<2>(ctx, P, S, nd, min_disp, uniq, diff, d_disp, dstride); break;
    default: sg_launch_select<4>(ctx, P, S, nd, min_disp, uniq, diff, d_disp, dstride); break;
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
