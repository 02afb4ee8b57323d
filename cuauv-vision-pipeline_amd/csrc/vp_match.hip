// cv2.matchTemplate, the six methods on uint8 images of 1..4 channels (tests/match_template_restate.py is the
// statement).  Every sum is an exact unsigned 32-bit integer; the arithmetic after them is double, in one fixed order, rounded to
// float32 once.  Four kernels, the geometry of all of them in vp_match_plan.h:
//
//   k_mt_template  one block: T2 = sum T^2, T1_c = sum T per channel, tn_int and templNorm into vp_match_stats, and the template in the
//                  form the correlation reads - rows of tpitch words, the bytes of a row as they lie (channels interleaved), zero bytes
//                  behind them.
//   k_mt_int_rows  one block per row: the running sums along the row of sum_c I^2 and of every channel of I, wrapping uint32, into
//                  rows 1..h of (h + 1) x (w + 1) integrals (row 0 and column 0 are zeros).  Only the planes the method reads.
//   k_mt_int_cols  the running sums down the columns, in place: a block takes MT_INT_COLS columns of one plane, each of its MT_INT_SEGS
//                  waves a segment of rows - its total first, then the segment again behind the totals of the waves above.  Window
//                  sums are below 2^32, so the four-corner difference of the wrapping integral is exact, whatever the window.
//   k_mt_corr      a block owns MT_TILE_W x MT_TILE_H results and walks the template in chunks; per chunk it stages the image patch
//                  and the template chunk in LDS.  A lane keeps MT_RX x MT_RY accumulators: one staged image word, shifted by
//                  v_alignbyte_b32 to the lane's MT_RX results, feeds MT_RX * MT_RY v_dot4_u32_u8, the template words wave-uniform.
//                  The epilogue reads the window sums and the statistics, does the double arithmetic and stores float32.
#include "vp_internal.h"
#include "vp_match_plan.h"

static_assert(MT_SQDIFF == VP_TM_SQDIFF && MT_SQDIFF_NORMED == VP_TM_SQDIFF_NORMED && MT_CCORR == VP_TM_CCORR && MT_CCORR_NORMED == VP_TM_CCORR_NORMED &&
                  MT_CCOEFF == VP_TM_CCOEFF && MT_CCOEFF_NORMED == VP_TM_CCOEFF_NORMED,
              "method codes of vp.h");

namespace {

// grid 1, 256 threads.  templ: th rows of tstride bytes, twb of them used; packed: th rows of tpitch words.
__global__ __launch_bounds__(256) void k_mt_template(const uint8_t* __restrict__ templ, size_t tstride, int twb, int th, int cn, int tpitch, int coeff_normed,
                                                     u32* __restrict__ packed, vp_match_stats* __restrict__ stats)
{
    __shared__ u64 sum[1 + MT_MAX_CN];
    if (threadIdx.x < 1 + MT_MAX_CN) sum[threadIdx.x] = 0;
    __syncthreads();
    u64 t2 = 0, t1[MT_MAX_CN] = {0, 0, 0, 0};
    const int words = th * tpitch;
    for (int i = threadIdx.x; i < words; i += 256) {
        const int row = i / tpitch, wd = i - row * tpitch;
        const uint8_t* p = templ + (size_t)row * tstride;
        u32 v = 0;
        for (int b = 0; b < 4; b++) {
            const int xb = 4 * wd + b;
            if (xb >= twb) break;
            const u32 t = p[xb];
            v |= t << (8 * b);
            t2 += (u64)t * t;
            const int c = xb % cn;
            for (int k = 0; k < MT_MAX_CN; k++) t1[k] += k == c ? t : 0;
        }
        packed[i] = v;
    }
    atomicAdd(&sum[0], t2);
    for (int k = 0; k < MT_MAX_CN; k++) atomicAdd(&sum[1 + k], t1[k]);
    __syncthreads();
    if (threadIdx.x == 0) {
        const u64 n = (u64)(twb / cn) * th;
        u64 tn = n * sum[0];
        stats->t2 = sum[0];
        for (int k = 0; k < MT_MAX_CN; k++) {
            stats->t1[k] = sum[1 + k];
            if (coeff_normed) tn -= sum[1 + k] * sum[1 + k];
        }
        stats->tn_int = tn;
        stats->templ_norm = __dsqrt_rn(__ddiv_rn((double)tn, (double)n));
    }
}

// inclusive sums of NV values per thread over the block's 256 threads, in thread order; *total: the sums of all 256
template <int NV>
__device__ __forceinline__ void mt_block_scan(u32 (&v)[NV], u32 (&total)[NV], u32 (*part)[4])
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int off = 1; off < 64; off <<= 1)
        for (int i = 0; i < NV; i++) {
            const u32 a = __shfl_up(v[i], off);
            if (lane >= off) v[i] += a;
        }
    __syncthreads();                                    // the last round's readers of part are done
    if (lane == 63)
        for (int i = 0; i < NV; i++) part[i][wv] = v[i];
    __syncthreads();
    for (int i = 0; i < NV; i++) {
        u32 before = 0, all = 0;
        for (int k = 0; k < 4; k++) {
            before += k < wv ? part[i][k] : 0;
            all += part[i][k];
        }
        v[i] += before;
        total[i] = all;
    }
}

// grid h + 1 (integral rows), 256 threads.  A: planes of (h + 1) * ipitch entries; plane 0 the squares when need_s2, then the channels
// when need_s1.
template <int CN>
__global__ __launch_bounds__(256) void k_mt_int_rows(const uint8_t* __restrict__ src, size_t stride, int w, int h, int need_s2, int need_s1, u32* __restrict__ A,
                                                     int ipitch)
{
    __shared__ u32 part[1 + CN][4];
    const size_t plane = (size_t)(h + 1) * ipitch;
    const int planes = need_s2 + need_s1 * CN;
    u32* row = A + (size_t)blockIdx.x * ipitch;
    if (blockIdx.x == 0) {
        for (int p = 0; p < planes; p++)
            for (int x = threadIdx.x; x <= w; x += 256) row[p * plane + x] = 0;
        return;
    }
    const uint8_t* s = src + (size_t)(blockIdx.x - 1) * stride;
    if (threadIdx.x == 0)
        for (int p = 0; p < planes; p++) row[p * plane] = 0;
    u32 carry[1 + CN];
    for (int i = 0; i <= CN; i++) carry[i] = 0;
    for (int x0 = 0; x0 < w; x0 += 256) {               // every thread takes every round: the scan synchronises the block
        const int x = x0 + threadIdx.x;
        u32 v[1 + CN], total[1 + CN];
        v[0] = 0;
        for (int c = 0; c < CN; c++) {
            const u32 t = x < w ? s[(size_t)x * CN + c] : 0;
            v[1 + c] = t;
            v[0] += t * t;
        }
        mt_block_scan<1 + CN>(v, total, part);
        if (x < w) {
            if (need_s2) row[x + 1] = carry[0] + v[0];
            if (need_s1)
                for (int c = 0; c < CN; c++) row[(size_t)(need_s2 + c) * plane + x + 1] = carry[1 + c] + v[1 + c];
        }
        for (int i = 0; i <= CN; i++) carry[i] += total[i];
    }
}

// grid (ceil((w + 1) / MT_INT_COLS), planes), 64 * MT_INT_SEGS threads
__global__ __launch_bounds__(64 * MT_INT_SEGS) void k_mt_int_cols(u32* __restrict__ A, int w, int h, int ipitch)
{
    __shared__ u32 tot[MT_INT_SEGS][MT_INT_COLS];
    const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6, x = blockIdx.x * MT_INT_COLS + lane;
    const int per = (h + MT_INT_SEGS - 1) / MT_INT_SEGS, ya = 1 + seg * per, yb = min(h + 1, ya + per);      // integral rows [ya, yb)
    u32* col = A + (size_t)blockIdx.y * (h + 1) * ipitch + x;
    u32 sum = 0;
    if (x <= w)
        for (int y = ya; y < yb; y++) sum += col[(size_t)y * ipitch];
    tot[seg][lane] = sum;
    __syncthreads();
    u32 run = 0;
    for (int k = 0; k < seg; k++) run += tot[k][lane];
    if (x <= w)
        for (int y = ya; y < yb; y++) {
            run += col[(size_t)y * ipitch];
            col[(size_t)y * ipitch] = run;
        }
}

// the word of image bytes xb .. xb + 3 of a row of rowbytes bytes: a byte past the row is never read and counts as 0
__device__ __forceinline__ u32 mt_load_word(const uint8_t* __restrict__ row, int xb, int rowbytes, int aligned)
{
    if (xb + 3 < rowbytes) {
        if (aligned) return *reinterpret_cast<const u32*>(row + xb);
        return (u32)row[xb] | ((u32)row[xb + 1] << 8) | ((u32)row[xb + 2] << 16) | ((u32)row[xb + 3] << 24);
    }
    u32 v = 0;
    for (int b = 0; b < 4; b++)
        if (xb + b < rowbytes) v |= (u32)row[xb + b] << (8 * b);
    return v;
}

struct mt_args {
    const uint8_t* src;        // rows of stride bytes, rowbytes = w * cn of them used
    size_t stride;
    int rowbytes, h, aligned;  // aligned: src and stride are multiples of 4
    const u32* templ;          // th rows of tpitch words
    int tw, th, tpitch;
    int patch_pitch, templ_off;
    int rw, rh, method, need_s1, need_s2;
    const u32* integral;       // planes of (h + 1) * ipitch entries
    int ipitch;
    const vp_match_stats* stats;
    float* dst;
    size_t dstride;            // in floats
};

__device__ __forceinline__ u32 mt_window(const u32* __restrict__ I, int ipitch, int x, int y, int tw, int th)
{
    const u32* a = I + (size_t)y * ipitch + x;
    const u32* b = a + (size_t)th * ipitch;
    return b[tw] - a[tw] - b[0] + a[0];
}

// steps 1 to 3 of the statement for one result pixel
template <int CN>
__device__ __forceinline__ float mt_finish(const mt_args& a, u32 corr, int x, int y)
{
    const vp_match_stats& st = *a.stats;
    const size_t plane = (size_t)(a.h + 1) * a.ipitch;
    const long long n = (long long)a.tw * a.th;
    const double dn = (double)n;
    u32 s2 = 0;
    if (a.need_s2) s2 = mt_window(a.integral, a.ipitch, x, y, a.tw, a.th);
    long long cross = 0, sq = 0;
    if (a.need_s1)
        for (int c = 0; c < CN; c++) {
            const long long s1 = mt_window(a.integral + (size_t)(a.need_s2 + c) * plane, a.ipitch, x, y, a.tw, a.th);
            cross += s1 * (long long)st.t1[c];
            sq += s1 * s1;
        }
    double num;
    long long d_int = n * (long long)s2;
    if (a.method == MT_CCORR || a.method == MT_CCORR_NORMED) {
        num = (double)corr;
    } else if (a.method == MT_SQDIFF || a.method == MT_SQDIFF_NORMED) {
        num = (double)((long long)s2 - 2ll * (long long)corr + (long long)st.t2);
    } else {
        num = __ddiv_rn((double)(n * (long long)corr - cross), dn);
        d_int -= sq;
    }
    if (!vp_match_normed(a.method)) return (float)num;
    if (a.method == MT_CCOEFF_NORMED && st.tn_int == 0) return 1.0f;
    const double diff2 = __ddiv_rn((double)d_int, dn);
    const double eps = (double)(10.0f * 1.1920928955078125e-07f) * (double)s2;
    double t = 0.0;
    if (!(diff2 <= (eps < 0.5 ? eps : 0.5))) t = __dsqrt_rn(diff2) * st.templ_norm;
    const double mag = num < 0.0 ? -num : num;
    if (mag < t) num = __ddiv_rn(num, t);
    else if (mag < t * 1.125) num = num > 0.0 ? 1.0 : -1.0;
    else num = a.method == MT_SQDIFF_NORMED ? 1.0 : 0.0;
    return (float)num;
}

// grid (plan.grid_x, plan.grid_y), MT_THREADS threads, plan.lds_bytes of dynamic LDS
template <int CN>
__global__ __launch_bounds__(MT_THREADS) void k_mt_corr(const mt_args a)
{
    constexpr int NW = ((MT_RX - 1) * CN) / 4;           // whole words between a lane's first and last result
    extern __shared__ __align__(16) u32 L[];
    u32* P = L;                                          // the image patch: rows of patch_pitch words
    u32* T = L + a.templ_off;                            // the template chunk: MT_RY - 1 zero rows, its rows, MT_RY - 1 zero rows; cw words each
    const int tx = threadIdx.x % MT_LANES_X, ty = threadIdx.x / MT_LANES_X;
    const int x0 = blockIdx.x * MT_TILE_W, y0 = blockIdx.y * MT_TILE_H;
    const int pp = a.patch_pitch;
    u32 acc[MT_RY][MT_RX];
    for (int i = 0; i < MT_RY; i++)
        for (int r = 0; r < MT_RX; r++) acc[i][r] = 0;

    for (int jc = 0; jc < a.th; jc += MT_CHUNK_ROWS) {
        const int cr = min(MT_CHUNK_ROWS, a.th - jc);
        for (int kc = 0; kc < a.tpitch; kc += MT_CHUNK_WORDS) {
            const int cw = min(MT_CHUNK_WORDS, a.tpitch - kc);
            const int prows = MT_TILE_H + cr - 1, pw = MT_LANES_X * CN + cw + MT_PATCH_SLACK;
            __syncthreads();                             // the chunk before has been read
            for (int i = threadIdx.x; i < prows * pw; i += MT_THREADS) {
                const int r = i / pw, c = i - r * pw, gy = y0 + jc + r;
                P[r * pp + c] = gy < a.h ? mt_load_word(a.src + (size_t)gy * a.stride, x0 * CN + 4 * (kc + c), a.rowbytes, a.aligned) : 0u;
            }
            for (int i = threadIdx.x; i < (cr + 2 * (MT_RY - 1)) * cw; i += MT_THREADS) {
                const int r = i / cw - (MT_RY - 1), c = i % cw;
                T[i] = r >= 0 && r < cr ? a.templ[(size_t)(jc + r) * a.tpitch + kc + c] : 0u;
            }
            __syncthreads();
            // patch row ty * MT_RY + d lies under template row d - ry of the chunk for the lane's result row ry
            for (int d = 0; d < cr + MT_RY - 1; d++) {
                const u32* prow = P + (ty * MT_RY + d) * pp + tx * CN;
                const u32* trow = T + (d + MT_RY - 1) * cw;
                for (int k = 0; k < cw; k += 4) {
                    u32 wd[NW + 5];
                    for (int c = 0; c < NW + 5; c++) wd[c] = prow[k + c];
                    uint4 tq[MT_RY];
                    for (int ry = 0; ry < MT_RY; ry++) tq[ry] = *reinterpret_cast<const uint4*>(trow - ry * cw + k);
#pragma unroll
                    for (int kk = 0; kk < 4; kk++)
#pragma unroll
                        for (int r = 0; r < MT_RX; r++) {
                            const int wi = (r * CN) >> 2, sh = (r * CN) & 3;
                            const u32 v = sh ? __builtin_amdgcn_alignbyte(wd[kk + wi + 1], wd[kk + wi], sh) : wd[kk + wi];
#pragma unroll
                            for (int ry = 0; ry < MT_RY; ry++) {
                                const u32 t = kk == 0 ? tq[ry].x : kk == 1 ? tq[ry].y : kk == 2 ? tq[ry].z : tq[ry].w;
                                acc[ry][r] = __builtin_amdgcn_udot4(v, t, acc[ry][r], false);
                            }
                        }
                }
            }
        }
    }

    for (int ry = 0; ry < MT_RY; ry++) {
        const int y = y0 + ty * MT_RY + ry;
        if (y >= a.rh) break;
        for (int r = 0; r < MT_RX; r++) {
            const int x = x0 + tx * MT_RX + r;
            if (x < a.rw) a.dst[(size_t)y * a.dstride + x] = mt_finish<CN>(a, acc[ry][r], x, y);
        }
    }
}

template <int CN>
void mt_launch(vp_ctx* ctx, const vp_match_plan& P, const mt_args& a, u32* d_int, int w)
{
    if (P.planes) {
        {
            vp_prof_scope ps(ctx, VPK_OTHER);
            hipLaunchKernelGGL((k_mt_int_rows<CN>), dim3((unsigned)(a.h + 1)), dim3(256), 0, ctx->stream, a.src, a.stride, w, a.h, P.need_s2, P.need_s1, d_int, P.ipitch);
        }
        {
            vp_prof_scope ps(ctx, VPK_OTHER);
            hipLaunchKernelGGL(k_mt_int_cols, dim3((unsigned)((w + 1 + MT_INT_COLS - 1) / MT_INT_COLS), (unsigned)P.planes), dim3(64 * MT_INT_SEGS), 0, ctx->stream,
                               d_int, w, a.h, P.ipitch);
        }
    }
    vp_prof_scope ps(ctx, VPK_OTHER);
    hipLaunchKernelGGL((k_mt_corr<CN>), dim3(P.grid_x, P.grid_y), dim3(MT_THREADS), P.lds_bytes, ctx->stream, a);
}

}  // namespace

// arguments as vp_match_template_refusal admitted them and P as vp_match_make_plan made it; d_ws: P.ws_bytes of workspace, 256-byte
// aligned; d_dst: rows of dstride bytes.  Two to four launches, enqueued.
int vpk_match_template(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int cn, const uint8_t* d_templ, size_t tstride, int tw, int th, int method,
                       const vp_match_plan& P, uint8_t* d_ws, float* d_dst, size_t dstride)
{
    vp_match_stats* d_stats = reinterpret_cast<vp_match_stats*>(d_ws + P.off_stats);
    u32* d_packed = reinterpret_cast<u32*>(d_ws + P.off_templ);
    u32* d_int = reinterpret_cast<u32*>(d_ws + P.off_integral);
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_mt_template, dim3(1), dim3(256), 0, ctx->stream, d_templ, tstride, P.twb, th, cn, P.tpitch, method == MT_CCOEFF_NORMED, d_packed, d_stats);
    }
    VP_HIP(ctx, hipGetLastError());
    mt_args a;
    a.src = d_src;
    a.stride = stride;
    a.rowbytes = w * cn;
    a.h = h;
    a.aligned = (uintptr_t)d_src % 4 == 0 && stride % 4 == 0;
    a.templ = d_packed;
    a.tw = tw;
    a.th = th;
    a.tpitch = P.tpitch;
    a.patch_pitch = P.patch_pitch;
    a.templ_off = P.templ_off;
    a.rw = P.rw;
    a.rh = P.rh;
    a.method = method;
    a.need_s1 = P.need_s1;
    a.need_s2 = P.need_s2;
    a.integral = d_int;
    a.ipitch = P.ipitch;
    a.stats = d_stats;
    a.dst = d_dst;
    a.dstride = dstride / 4;
    switch (cn) {
        case 1: mt_launch<1>(ctx, P, a, d_int, w); break;
        case 2: mt_launch<2>(ctx, P, a, d_int, w); break;
        case 3: mt_launch<3>(ctx, P, a, d_int, w); break;
        default: mt_launch<4>(ctx, P, a, d_int, w); break;
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
