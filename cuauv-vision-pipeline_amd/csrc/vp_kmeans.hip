// Colour k-means on uint8 images (the statement: tests/kmeans_restate.py; sizes, bounds and the table's layout:
// vp_kmeans_plan.h).  Every pass assigns each pixel to the nearest centre - squared distances in double, every operation an explicit
// round-to-nearest intrinsic, the lowest index on ties - and sums n, S1 = sum p and S2 = sum p^2 per cluster as exact integers, so
// the result does not depend on the order in which the device adds.  The loop lives on the device: a state word says whether the next
// pass is followed by an update, is the last one, or has nothing left to do, and the host enqueues max_iter rounds without looking.
#include "vp_internal.h"
#include "vp_kmeans_plan.h"

// d_k of one pixel against one centre, in channel order
template <int CN>
__device__ __forceinline__ double km_dist(const uint8_t* p, const double* c)
{
    double d = 0.0;
#pragma unroll
    for (int ch = 0; ch < CN; ch++) {
        const double t = __dsub_rn((double)p[ch], c[ch]);
        d = __dadd_rn(d, __dmul_rn(t, t));
    }
    return d;
}

// One launch zeroes the sums, resets the state words and writes the initial centres: the given ones, or the pixels at the seed indices.
__global__ __launch_bounds__(KM_THREADS) void k_km_init(const uint8_t* __restrict__ src, size_t stride, int w, int cn, int k, const float* __restrict__ cinit,
                                                         const int32_t* __restrict__ seeds, u32* __restrict__ state, float* __restrict__ centres,
                                                         u32* __restrict__ cnt, u32* __restrict__ s1, u64* __restrict__ s2)
{
    const int t = threadIdx.x;
    if (t < 4) state[t] = 0;        // KM_RUNNING, no pass yet
    if (t < k) cnt[t] = 0;
    for (int i = t; i < k * cn; i += KM_THREADS) {
        s1[i] = 0;
        s2[i] = 0;
        if (cinit) centres[i] = cinit[i];
        else {
            const int s = seeds[i / cn], y = s / w, x = s - y * w;
            centres[i] = (float)src[(size_t)y * stride + (size_t)x * cn + (i % cn)];
        }
    }
}

// LABELS false: one assign-and-reduce pass.  The centres sit in LDS as doubles; a lane takes KM_PX neighbouring pixels of a row
// KM_ITERS times and keeps the sums of its current run of equal labels in registers.  A pixel with another label sends the run to
// the block's LDS table with per-lane atomics.  What every lane still holds at the end goes in one of two ways: when a ballot shows
// one label for the whole wave, the lanes' sums are reduced across the wave and one lane adds them; otherwise every lane adds its
// own.  The table is flushed to the device sums once per block.  LABELS true: the same argmin, written out; no sums.
template <int CN, bool LABELS>
__global__ __launch_bounds__(KM_THREADS) void k_km_assign(const uint8_t* __restrict__ src, size_t stride, int w, int h, int k, const u32* __restrict__ state,
                                                           const float* __restrict__ centres, u32* __restrict__ cnt, u32* __restrict__ s1,
                                                           u64* __restrict__ s2, int32_t* __restrict__ labels, size_t lstride)
{
    __shared__ double s_c[KM_MAX_K * CN];
    __shared__ u32 s_tab[LABELS ? 1 : KM_MAX_K * (1 + 2 * CN)];
    const int tid = threadIdx.x;
    if (!LABELS && state[0] == KM_DONE) return;       // the same word for every lane of the grid
    for (int i = tid; i < k * CN; i += KM_THREADS) s_c[i] = (double)centres[i];
    if (!LABELS)
        for (int i = tid; i < k * (1 + 2 * CN); i += KM_THREADS) s_tab[i] = 0;
    __syncthreads();
    u32* t_n = s_tab;
    u32* t_s1 = s_tab + k;
    u32* t_s2 = s_tab + k + k * CN;

    const u32 cpr = (u32)(w + KM_PX - 1) / KM_PX, total = cpr * (u32)h;
    int cur = -1;                       // the label of the run this lane holds
    u32 rn = 0, r1[CN], r2[CN];
#pragma unroll
    for (int ch = 0; ch < CN; ch++) r1[ch] = r2[ch] = 0;

    for (int it = 0; it < KM_ITERS; it++) {
        const u32 c = blockIdx.x * KM_BLOCK_CHUNKS + (u32)it * KM_THREADS + (u32)tid;
        if (c >= total) continue;
        const u32 y = c / cpr, x0 = (c - y * cpr) * KM_PX;
        const int npx = (int)(w - x0) < KM_PX ? (int)(w - x0) : KM_PX;
        const uint8_t* row = src + (size_t)y * stride + (size_t)x0 * CN;
        union { u32 wd[CN]; uint8_t b[KM_PX * CN]; } px;
        if (npx == KM_PX && ((uintptr_t)row & 3) == 0) {
#pragma unroll
            for (int i = 0; i < CN; i++) px.wd[i] = reinterpret_cast<const u32*>(row)[i];
        } else {
#pragma unroll
            for (int i = 0; i < KM_PX * CN; i++) px.b[i] = i < npx * CN ? row[i] : (uint8_t)0;
        }
        double best[KM_PX];
        int lab[KM_PX];
#pragma unroll
        for (int j = 0; j < KM_PX; j++) {
            best[j] = km_dist<CN>(px.b + j * CN, s_c);
            lab[j] = 0;
        }
        for (int kk = 1; kk < k; kk++) {
            double cc[CN];
#pragma unroll
            for (int ch = 0; ch < CN; ch++) cc[ch] = s_c[kk * CN + ch];
#pragma unroll
            for (int j = 0; j < KM_PX; j++) {
                const double d = km_dist<CN>(px.b + j * CN, cc);
                if (d < best[j]) { best[j] = d; lab[j] = kk; }
            }
        }
        if (LABELS) {
            int32_t* out = labels + (size_t)y * lstride + x0;
            if (npx == KM_PX && ((uintptr_t)out & 15) == 0) vp_store16(out, (u32)lab[0], (u32)lab[1], (u32)lab[2], (u32)lab[3]);
            else {
#pragma unroll
                for (int j = 0; j < KM_PX; j++)
                    if (j < npx) out[j] = lab[j];
            }
            continue;
        }
#pragma unroll
        for (int j = 0; j < KM_PX; j++) {
            if (j >= npx) break;
            if (lab[j] != cur) {
                if (rn) {                                       // the run ends: per-lane atomics into the block's table
                    atomicAdd(&t_n[cur], rn);
#pragma unroll
                    for (int ch = 0; ch < CN; ch++) {
                        atomicAdd(&t_s1[cur * CN + ch], r1[ch]);
                        atomicAdd(&t_s2[cur * CN + ch], r2[ch]);
                        r1[ch] = r2[ch] = 0;
                    }
                    rn = 0;
                }
                cur = lab[j];
            }
            rn++;
#pragma unroll
            for (int ch = 0; ch < CN; ch++) {
                const u32 v = px.b[j * CN + ch];
                r1[ch] += v;
                r2[ch] += v * v;
            }
        }
    }
    if (LABELS) return;

    // what the lanes still hold: every lane of the wave is here (no lane has left), so the ballots see all 64
    const u64 holders = __ballot(rn != 0);
    if (holders) {
        const int first = __ffsll((long long)holders) - 1;
        const int lab0 = __shfl(cur, first, 64);
        if (__ballot(rn != 0 && cur != lab0) == 0) {            // one label in the whole wave: reduce across lanes, one lane adds
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                rn += __shfl_xor(rn, m, 64);
#pragma unroll
                for (int ch = 0; ch < CN; ch++) {
                    r1[ch] += __shfl_xor(r1[ch], m, 64);
                    r2[ch] += __shfl_xor(r2[ch], m, 64);
                }
            }
            if ((tid & 63) == 0) {
                atomicAdd(&t_n[lab0], rn);
#pragma unroll
                for (int ch = 0; ch < CN; ch++) {
                    atomicAdd(&t_s1[lab0 * CN + ch], r1[ch]);
                    atomicAdd(&t_s2[lab0 * CN + ch], r2[ch]);
                }
            }
        } else if (rn) {                                        // mixed: every lane adds its own
            atomicAdd(&t_n[cur], rn);
#pragma unroll
            for (int ch = 0; ch < CN; ch++) {
                atomicAdd(&t_s1[cur * CN + ch], r1[ch]);
                atomicAdd(&t_s2[cur * CN + ch], r2[ch]);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < k; i += KM_THREADS)
        if (t_n[i]) atomicAdd(&cnt[i], t_n[i]);
    for (int i = tid; i < k * CN; i += KM_THREADS) {
        if (t_s1[i]) atomicAdd(&s1[i], t_s1[i]);
        if (t_s2[i]) atomicAdd(reinterpret_cast<unsigned long long*>(&s2[i]), (unsigned long long)t_s2[i]);
    }
}

// One block, one thread per cluster.  Counts the assign pass that has just run; ends the run when that was the last one (max_iter
// reached, or the pass after convergence); otherwise moves every centre to its cluster's mean - one correctly rounded double division,
// one rounding to float32, an empty cluster keeps its centre -, clears the sums for the next pass and compares the largest squared
// shift with eps^2.
__global__ __launch_bounds__(KM_THREADS) void k_km_update(int k, int cn, int max_iter, double eps2, u32* __restrict__ state, float* __restrict__ centres,
                                                           u32* __restrict__ cnt, u32* __restrict__ s1, u64* __restrict__ s2)
{
    __shared__ double s_shift[KM_THREADS];
    const int t = threadIdx.x;
    const u32 st = state[0], passes = state[1] + 1;
    __syncthreads();                    // every lane has read the two words before one of them is written
    if (st == KM_DONE) return;
    if ((int)passes == max_iter || st == KM_LAST) {
        if (t == 0) {
            state[0] = KM_DONE;
            state[1] = passes;
        }
        return;
    }
    double shift = 0.0;
    if (t < k) {
        const u32 n = cnt[t];
        for (int ch = 0; ch < cn; ch++) {
            const int i = t * cn + ch;
            const float old = centres[i];
            const float now = n ? __double2float_rn(__ddiv_rn((double)s1[i], (double)n)) : old;
            const double d = __dsub_rn((double)now, (double)old);
            shift = __dadd_rn(shift, __dmul_rn(d, d));
            centres[i] = now;
            s1[i] = 0;
            s2[i] = 0;
        }
        cnt[t] = 0;
    }
    s_shift[t] = shift;
    __syncthreads();
    for (int m = KM_THREADS / 2; m >= 1; m >>= 1) {
        if (t < m) s_shift[t] = s_shift[t] < s_shift[t + m] ? s_shift[t + m] : s_shift[t];
        __syncthreads();
    }
    if (t == 0) {
        state[0] = s_shift[0] <= eps2 ? KM_LAST : KM_RUNNING;
        state[1] = passes;
    }
}

struct km_select { uint8_t on[KM_MAX_K]; };

// mask = 255 where select[label] != 0; a wave holds 64 neighbouring pixels of a row, so its ballot is one word of the bit plane
__global__ __launch_bounds__(256) void k_label_select(const int32_t* __restrict__ labels, size_t lstride, int w, int k, km_select sel, uint8_t* __restrict__ mask,
                                                      size_t mstride, u64* __restrict__ bits)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    bool on = false;
    if (x < w) {
        const int l = labels[(size_t)y * lstride + x];
        on = l >= 0 && l < k && sel.on[l] != 0;
        mask[(size_t)y * mstride + x] = on ? 255 : 0;
    }
    if (bits) {                          // w % 64 == 0: a wave is inside the row or outside it as a whole
        const u64 word = __ballot(on);
        if ((threadIdx.x & 63) == 0 && x < w) bits[(size_t)y * (w / 64) + x / 64] = word;
    }
}

template <bool LABELS>
static void km_launch_assign(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int cn, int k, const u32* state, const float* centres, u32* cnt,
                             u32* s1, u64* s2, int32_t* d_labels, size_t lstride)
{
    const dim3 grid(vp_kmeans_blocks(w, h)), block(KM_THREADS);
    vp_prof_scope ps(ctx, VPK_OTHER);
    switch (cn) {
    case 1: hipLaunchKernelGGL((k_km_assign<1, LABELS>), grid, block, 0, ctx->stream, d_src, stride, w, h, k, state, centres, cnt, s1, s2, d_labels, lstride); break;
    case 2: hipLaunchKernelGGL((k_km_assign<2, LABELS>), grid, block, 0, ctx->stream, d_src, stride, w, h, k, state, centres, cnt, s1, s2, d_labels, lstride); break;
    case 3: hipLaunchKernelGGL((k_km_assign<3, LABELS>), grid, block, 0, ctx->stream, d_src, stride, w, h, k, state, centres, cnt, s1, s2, d_labels, lstride); break;
    default: hipLaunchKernelGGL((k_km_assign<4, LABELS>), grid, block, 0, ctx->stream, d_src, stride, w, h, k, state, centres, cnt, s1, s2, d_labels, lstride); break;
    }
}

int vpk_kmeans(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int cn, int k, const float* d_cinit, const int32_t* d_seeds, int max_iter,
               double eps, uint8_t* d_table, int32_t* d_labels, size_t lstride)
{
    u64* s2 = reinterpret_cast<u64*>(d_table + vp_kmeans_off_s2(k, cn));
    u32* state = reinterpret_cast<u32*>(d_table + vp_kmeans_off_state(k, cn));
    float* centres = reinterpret_cast<float*>(d_table + vp_kmeans_off_centres(k, cn));
    u32* cnt = reinterpret_cast<u32*>(d_table + vp_kmeans_off_n(k, cn));
    u32* s1 = reinterpret_cast<u32*>(d_table + vp_kmeans_off_s1(k, cn));
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_km_init, dim3(1), dim3(KM_THREADS), 0, ctx->stream, d_src, stride, w, cn, k, d_cinit, d_seeds, state, centres, cnt, s1, s2);
    }
    const double eps2 = eps * eps;
    for (int i = 0; i < max_iter; i++) {
        km_launch_assign<false>(ctx, d_src, stride, w, h, cn, k, state, centres, cnt, s1, s2, nullptr, 0);
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_km_update, dim3(1), dim3(KM_THREADS), 0, ctx->stream, k, cn, max_iter, eps2, state, centres, cnt, s1, s2);
    }
    if (d_labels) km_launch_assign<true>(ctx, d_src, stride, w, h, cn, k, state, centres, cnt, s1, s2, d_labels, lstride);
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

int vpk_label_select(vp_ctx* ctx, const int32_t* d_labels, size_t lstride, int w, int h, const uint8_t* select, int k, uint8_t* d_mask, size_t mstride, u64* d_bits)
{
    km_select sel;
    for (int i = 0; i < KM_MAX_K; i++) sel.on[i] = i < k ? select[i] : 0;
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_label_select, dim3((unsigned)((w + 255) / 256), (unsigned)h), dim3(256), 0, ctx->stream, d_labels, lstride, w, k, sel, d_mask, mstride,
                           w % 64 == 0 ? d_bits : nullptr);
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
