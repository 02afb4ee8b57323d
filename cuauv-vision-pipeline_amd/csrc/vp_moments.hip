// Spatial moments up to order three, as exact integers: of a uint8 image or of a mask's bit plane (k_moments_u8), and of every
// component of an int32 label image at once (k_label_moments_i32).  Order everywhere: m00 m10 m01 m20 m11 m02 m30 m21 m12 m03,
// m_pq = sum x^p y^q v.  All sums are unsigned 64-bit; the callers have refused sizes whose worst case reaches 2^63
// (vp_moments_plan.h), so nothing wraps and the order of the additions - lanes, waves, blocks, atomics - cannot show in the result.
#include "vp_internal.h"
#include "vp_moments_plan.h"
#include <limits.h>

// the ten moments of one row from its four x sums s_p = sum x^p v: m_pq += y^q s_p
__device__ __forceinline__ void mm_row(u64* acc, u64 y, u64 r0, u64 r1, u64 r2, u64 r3)
{
    const u64 y2 = y * y, y3 = y2 * y;
    acc[0] += r0;       acc[1] += r1;       acc[2] += y * r0;
    acc[3] += r2;       acc[4] += y * r1;   acc[5] += y2 * r0;
    acc[6] += r3;       acc[7] += y * r2;   acc[8] += y2 * r1;   acc[9] += y3 * r0;
}

// One wave takes MM_SPAN bytes (BITS: 64 words) of a row, one block MM_ROWS rows.  A lane's 16 pixels (64 bits) are summed in
// coordinates local to its chunk, t = 0 .. 15 (63), in 32 bits - at most 255 * sum t^3 = 255 * 14400 (sum t^3 = 4064256 over 64 bits) -
// and moved to the chunk's place in the row, x = xo + t, by the binomial in 64 bits.  Byte rows are cut at 16-byte ADDRESSES, not
// columns: the chunk that holds the row's first pixel starts up to 15 bytes before it (xo < 0) and is read byte by byte, like the
// last one; every chunk in between is one aligned 16-byte load, whatever the stride and the pointer.
template <int BITS>
__global__ __launch_bounds__(MM_TB) void k_moments_u8(const uint8_t* __restrict__ src, size_t stride, const u64* __restrict__ bits, int ww, int w, int h,
                                                      int binary, u64* __restrict__ out)
{
    __shared__ u64 part[MM_TB / 64][10];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 acc[10];
#pragma unroll
    for (int k = 0; k < 10; k++) acc[k] = 0;
    for (int r = wave; r < MM_ROWS; r += MM_TB / 64) {
        const int y = (int)blockIdx.y * MM_ROWS + r;
        if (y >= h) break;
        u32 s0 = 0, s1 = 0, s2 = 0, s3 = 0;
        long long xo;
        if (BITS) {
            const int k = (int)blockIdx.x * 64 + lane;
            xo = (long long)k * 64;
            u64 wv = 0;
            if (k < ww) {
                wv = bits[(size_t)y * ww + k];
                const int left = w - k * 64;                     // >= 1: k < ww
                if (left < 64) wv &= (1ull << left) - 1;         // bits past the row's end do not count, whatever they hold
            }
#pragma unroll
            for (int t = 0; t < 64; t++) {
                const u32 b = (u32)(wv >> t) & 1u;
                s0 += b; s1 += b * (u32)t; s2 += b * (u32)(t * t); s3 += b * (u32)(t * t * t);
            }
        } else {
            const uint8_t* row = src + (size_t)y * stride;
            const int a = (int)((uintptr_t)row & 15);
            xo = ((long long)blockIdx.x * 64 + lane) * MM_CHUNK - a;      // >= -15
            u32 v[MM_CHUNK];
#pragma unroll
            for (int t = 0; t < MM_CHUNK; t++) v[t] = 0;
            if (xo >= 0 && xo + MM_CHUNK <= w) {
                const uint4 q = *reinterpret_cast<const uint4*>(row + xo);
                const u32 qq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int t = 0; t < MM_CHUNK; t++) v[t] = (qq[t >> 2] >> (8 * (t & 3))) & 255u;
            } else if (xo < w) {
#pragma unroll
                for (int t = 0; t < MM_CHUNK; t++) {
                    const long long x = xo + t;
                    if (x >= 0 && x < w) v[t] = row[x];
                }
            }
#pragma unroll
            for (int t = 0; t < MM_CHUNK; t++) {
                const u32 b = binary ? (u32)(v[t] != 0) : v[t];
                s0 += b; s1 += b * (u32)t; s2 += b * (u32)(t * t); s3 += b * (u32)(t * t * t);
            }
        }
        // x^p = (xo + t)^p; modulo 2^64 throughout, so a negative xo needs no care: the true sums are not negative
        const u64 X = (u64)xo, X2 = X * X, X3 = X2 * X;
        u64 r0 = s0;
        u64 r1 = s1 + X * s0;
        u64 r2 = s2 + 2 * X * s1 + X2 * s0;
        u64 r3 = s3 + 3 * X * s2 + 3 * X2 * s1 + X3 * s0;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            r0 += __shfl_xor(r0, off);
            r1 += __shfl_xor(r1, off);
            r2 += __shfl_xor(r2, off);
            r3 += __shfl_xor(r3, off);
        }
        mm_row(acc, (u64)y, r0, r1, r2, r3);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 10; k++) part[wave][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < 10) {
        u64 t = 0;
#pragma unroll
        for (int i = 0; i < MM_TB / 64; i++) t += part[i][threadIdx.x];
        if (t) atomicAdd(&out[threadIdx.x], t);
    }
}

// sums of x^p over a <= x < b from the closed forms P_p(n) = sum_{x < n} x^p (n = 0: every product has a zero factor)
__device__ __forceinline__ u64 lm_p1(u64 n) { return n * (n - 1) / 2; }
__device__ __forceinline__ u64 lm_p2(u64 n) { return (n - 1) * n * (2 * n - 1) / 6; }

// the run [a, b) of row y into row `label` of the table - the block's own for labels below lds_rows, the device's for the others; a
// label outside 0 .. nlabels - 1 is never used as an index
__device__ __forceinline__ void lm_add(u64* lds_tab, int lds_rows, u64* table, int label, int nlabels, int a, int b, int y)
{
    if ((u32)label >= (u32)nlabels || b <= a) return;
    const u64 ua = (u64)a, ub = (u64)b, uy = (u64)y;
    const u64 r0 = ub - ua, r1 = lm_p1(ub) - lm_p1(ua), r2 = lm_p2(ub) - lm_p2(ua);
    const u64 ta = lm_p1(ua), tb = lm_p1(ub), r3 = tb * tb - ta * ta;
    u64 m[10];
#pragma unroll
    for (int k = 0; k < 10; k++) m[k] = 0;
    mm_row(m, uy, r0, r1, r2, r3);
    if (label < lds_rows) {
        u64* rowp = lds_tab + label * 10;
#pragma unroll
        for (int k = 0; k < 10; k++)
            if (m[k]) atomicAdd(&rowp[k], m[k]);
    } else {
        u64* rowp = table + (size_t)label * 10;
#pragma unroll
        for (int k = 0; k < 10; k++)
            if (m[k]) atomicAdd(&rowp[k], m[k]);
    }
}

// One wave walks LM_SPAN pixels of a row, 64 at a time; one block LM_ROWS rows.  A lane whose label differs from its left neighbour's
// is a run head (ballot); the head closes the run BEFORE it - that run began at the previous head of this step or, with none, where the
// wave's open run began in an earlier step - and the run that reaches the end of the step stays open.  Lanes past the row's end carry
// INT_MIN, which closes the last run and counts nowhere.  The first lds_rows rows of the table (<= nlabels, <= LM_LDS_LABELS; the
// launch brings lds_rows * 80 bytes of LDS) are the block's own, zeroed, then flushed with device atomics where not zero; a run of any
// other label is a device atomic at once.
__global__ __launch_bounds__(MM_TB) void k_label_moments_i32(const int32_t* __restrict__ lab, size_t stride_el, int w, int h, int nlabels, int lds_rows,
                                                             u64* __restrict__ table)
{
    extern __shared__ u64 lm_tab[];
    for (int i = threadIdx.x; i < lds_rows * 10; i += MM_TB) lm_tab[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int xs0 = (int)blockIdx.x * LM_SPAN;
    const int xs1 = w - xs0 < LM_SPAN ? w : xs0 + LM_SPAN;
    for (int r = wave; r < LM_ROWS; r += MM_TB / 64) {
        const int y = (int)blockIdx.y * LM_ROWS + r;
        if (y >= h) break;
        const int32_t* row = lab + (size_t)y * stride_el;
        int open_label = 0, open_start = xs0;
        bool has_open = false;
        for (int xb = xs0; xb < xs1; xb += 64) {
            const int x = xb + lane;
            const int l = x < xs1 ? row[x] : INT_MIN;
            int prev = __shfl_up(l, 1);
            if (lane == 0) prev = open_label;
            const bool head = l != prev || (lane == 0 && !has_open);
            const u64 heads = __ballot(head);
            if (head && (lane > 0 || has_open)) {
                const u64 below = heads & ((1ull << lane) - 1);
                const int start = below ? xb + 63 - __clzll(below) : open_start;
                lm_add(lm_tab, lds_rows, table, prev, nlabels, start, x, y);
            }
            if (heads) open_start = xb + 63 - __clzll(heads);
            has_open = true;
            open_label = __shfl(l, 63);
        }
        if (lane == 0) lm_add(lm_tab, lds_rows, table, open_label, nlabels, open_start, xs1, y);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < lds_rows * 10; i += MM_TB) {
        const u64 v = lm_tab[i];
        if (v) atomicAdd(&table[i], v);
    }
}

// d_out10 is zeroed here; d_bits (nullable): the mask's bit plane, read instead of its bytes (binary only)
int vpk_moments_u8(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int binary, const u64* d_bits, u64* d_out10)
{
    VP_HIP(ctx, hipMemsetAsync(d_out10, 0, 10 * sizeof(u64), ctx->stream));
    if (d_bits) {
        const int ww = vp_ww(w);
        const dim3 grid((unsigned)((ww + 63) / 64), (unsigned)((h + MM_ROWS - 1) / MM_ROWS));
        hipLaunchKernelGGL(k_moments_u8<1>, grid, dim3(MM_TB), 0, ctx->stream, nullptr, (size_t)0, d_bits, ww, w, h, 1, d_out10);
    } else {
        const int chunks = (w + 2 * MM_CHUNK - 2) / MM_CHUNK;          // a row that starts 15 bytes into a chunk: ceil((w + 15) / 16)
        const dim3 grid((unsigned)((chunks + 63) / 64), (unsigned)((h + MM_ROWS - 1) / MM_ROWS));
        hipLaunchKernelGGL(k_moments_u8<0>, grid, dim3(MM_TB), 0, ctx->stream, d_src, stride, nullptr, 0, w, h, binary, d_out10);
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

// rows of the table a block keeps in LDS: all of them when they fit, else the first LM_HOT_LABELS - the background, label 0, is the
// one row every block adds to, and measured alone it serialises the device atomics; 0 with VP_OPT_LABEL_MOMENTS_LDS 0
int vp_label_moments_lds_rows(const vp_ctx* ctx, int nlabels)
{
    if (ctx->opt.v[VP_OPT_LABEL_MOMENTS_LDS] == 0) return 0;
    if (nlabels <= LM_LDS_LABELS) return nlabels;
    return LM_HOT_LABELS;
}

// d_table: (nlabels, 10) u64, zeroed here; stride in bytes, a multiple of 4
int vpk_label_moments_i32(vp_ctx* ctx, const int32_t* d_labels, size_t stride, int w, int h, int nlabels, u64* d_table)
{
    VP_HIP(ctx, hipMemsetAsync(d_table, 0, (size_t)nlabels * 10 * sizeof(u64), ctx->stream));
    const dim3 grid((unsigned)((w + LM_SPAN - 1) / LM_SPAN), (unsigned)((h + LM_ROWS - 1) / LM_ROWS));
    const int lds_rows = vp_label_moments_lds_rows(ctx, nlabels);
    hipLaunchKernelGGL(k_label_moments_i32, grid, dim3(MM_TB), (size_t)lds_rows * 10 * sizeof(u64), ctx->stream, d_labels, stride / 4, w, h, nlabels, lds_rows,
                       d_table);
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
