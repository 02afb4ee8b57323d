// Robust motion estimation from point pairs on the GPU: the RANSAC search of cv2.findHomography, estimateAffine2D and
// estimateAffinePartial2D as tests/model_restate.py states it (sampler, degeneracy tests, solvers, the inlier
// test and the plan: vp_model_plan.h).  A call enqueues, per round of RS_ROUND hypotheses, one scoring launch and one one-block launch
// that picks the round's best, folds it into the running best, compares it with the host's stop table and forms the next round's
// hypotheses; once the `done` word is set every later launch returns at once.  A last launch writes the inlier bytes of the best
// model.  Counts are integers added with integer atomics, so nothing depends on the order blocks run in.  This unit is compiled
// without floating-point contraction.
#include "vp_internal.h"
#include "vp_model_plan.h"
#include "vp_ransac_dev.h"

// (x, y) of both arrays side by side: what every other kernel reads
__global__ __launch_bounds__(RS_THREADS) void k_rs_pack(const float2* __restrict__ src, const float2* __restrict__ dst, int n, float4* __restrict__ pts)
{
    const int i = blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= n) return;
    const float2 a = src[i], b = dst[i];
    pts[i] = make_float4(a.x, a.y, b.x, b.y);
}

// One block, one thread per hypothesis of a round.  round >= 0: closes that round - the best count with the lowest index, folded
// into the running best (a later round has to be strictly better), then the comparison with need[round].  Unless the search has
// ended, forms the hypotheses of round + 1 and clears their counts.  round == -1 starts a call.
__global__ __launch_bounds__(RS_THREADS) void k_rs_select(const float4* __restrict__ pts, int n, int model, u32 seed, int max_iters, int round, int rounds,
                                                          const int32_t* __restrict__ need, vp_rs_state* __restrict__ state, int32_t* __restrict__ counts,
                                                          int32_t* __restrict__ valid, double* __restrict__ models)
{
    __shared__ u32 s_key[RS_THREADS];
    __shared__ int s_done;
    const int t = threadIdx.x;
    if (round < 0) {
        if (t == 0) {
            state->done = 0;
            state->rounds = 0;
            state->best_count = -1;
            state->best_j = -1;
            for (int k = 0; k < 9; k++) state->best[k] = 0.0;
            s_done = 0;
        }
    } else {
        if (state->done) return;             // the same word in every thread: all return or none
        const int c = valid[t] ? counts[t] : -1;
        const u32 top = vp_rsd_block_max<RS_THREADS>(s_key, t, ((u32)(c + 1) << 8) | (u32)(RS_THREADS - 1 - t));
        if (t == 0) {
            const int bc = (int)(top >> 8) - 1, bt = RS_THREADS - 1 - (int)(top & 255u);
            int best = state->best_count;
            if (bc > best) {
                best = bc;
                state->best_count = bc;
                state->best_j = round * RS_ROUND + bt;
                for (int k = 0; k < 9; k++) state->best[k] = models[bt * 9 + k];
            }
            state->rounds = round + 1;
            s_done = best >= need[round] || round + 1 >= rounds;
            state->done = s_done;
        }
    }
    __syncthreads();
    if (s_done) return;
    const int j = (round + 1) * RS_ROUND + t;
    int32_t s[4];
    double H[9];
    int ok = 0;
    if (j < max_iters) ok = vp_rs_hypothesis(reinterpret_cast<const float*>(pts), reinterpret_cast<const float*>(pts) + 2, 4, n, model, seed, (u32)j, s, H);
    valid[t] = ok;
    counts[t] = 0;
    for (int k = 0; k < 9; k++) models[t * 9 + k] = H[k];
}

// grid (RS_ROUND / RS_HYP_PER_BLOCK, chunks of RS_STAGE points): the block stages its chunk in LDS once, then each of its four waves
// tests it against every fourth hypothesis of the block's group - a ballot per 64 points, one integer add per wave and hypothesis
__global__ __launch_bounds__(RS_THREADS) void k_rs_score(const float4* __restrict__ pts, int n, int model, double t2, const vp_rs_state* __restrict__ state,
                                                         const int32_t* __restrict__ valid, const double* __restrict__ models, int32_t* __restrict__ counts)
{
    __shared__ float4 s_pts[RS_STAGE];
    if (state->done) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int base = blockIdx.y * RS_STAGE;
    const int cnt = n - base < RS_STAGE ? n - base : RS_STAGE;
    for (int i = tid; i < cnt; i += RS_THREADS) s_pts[i] = pts[base + i];
    __syncthreads();
    const int h0 = blockIdx.x * RS_HYP_PER_BLOCK;
    for (int h = h0 + wave; h < h0 + RS_HYP_PER_BLOCK; h += RS_THREADS / 64) {
        if (!valid[h]) continue;
        double H[9];
#pragma unroll
        for (int k = 0; k < 9; k++) H[k] = models[h * 9 + k];
        int c = 0;
        for (int i0 = 0; i0 < cnt; i0 += 64) {
            const int i = i0 + lane;
            bool in = false;
            if (i < cnt) {
                const float4 p = s_pts[i];
                in = vp_rs_inlier(H, model, (double)p.x, (double)p.y, (double)p.z, (double)p.w, t2);
            }
            c += __popcll(__ballot(in));
        }
        if (lane == 0 && c) atomicAdd(&counts[h], c);
    }
}

// the inlier bytes of the best model; zeros when the search found none
__global__ __launch_bounds__(RS_THREADS) void k_rs_mask(const float4* __restrict__ pts, int n, int model, int m, double t2, const vp_rs_state* __restrict__ state,
                                                        uint8_t* __restrict__ mask)
{
    const int i = blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= n) return;
    bool in = false;
    if (state->best_count >= m) {
        double H[9];
#pragma unroll
        for (int k = 0; k < 9; k++) H[k] = state->best[k];
        const float4 p = pts[i];
        in = vp_rs_inlier(H, model, (double)p.x, (double)p.y, (double)p.z, (double)p.w, t2);
    }
    mask[i] = in ? 1 : 0;
}

int vpk_rs_pack(vp_ctx* ctx, const float* d_src, const float* d_dst, int n, float* d_pts)
{
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_rs_pack, dim3((unsigned)((n + RS_THREADS - 1) / RS_THREADS)), dim3(RS_THREADS), 0, ctx->stream, reinterpret_cast<const float2*>(d_src),
                           reinterpret_cast<const float2*>(d_dst), n, reinterpret_cast<float4*>(d_pts));
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

int vpk_rs_search(vp_ctx* ctx, const vp_rs_plan& P, uint8_t* d_ws, int n, int model, double t2, int max_iters, u32 seed)
{
    const float4* pts = reinterpret_cast<const float4*>(d_ws);
    const int32_t* need = reinterpret_cast<const int32_t*>(d_ws + P.off_need);
    int32_t* counts = reinterpret_cast<int32_t*>(d_ws + P.off_counts);
    int32_t* valid = reinterpret_cast<int32_t*>(d_ws + P.off_valid);
    double* models = reinterpret_cast<double*>(d_ws + P.off_models);
    vp_rs_state* state = reinterpret_cast<vp_rs_state*>(d_ws + P.off_state);
    for (int r = -1; r < P.rounds; r++) {
        if (r >= 0) {
            vp_prof_scope ps(ctx, VPK_OTHER);
            hipLaunchKernelGGL(k_rs_score, dim3(P.score_gx, P.score_gy), dim3(RS_THREADS), 0, ctx->stream, pts, n, model, t2, state, valid, models, counts);
        }
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_rs_select, dim3(1), dim3(RS_THREADS), 0, ctx->stream, pts, n, model, seed, max_iters, r, P.rounds, need, state, counts, valid, models);
    }
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_rs_mask, dim3(P.mask_grid), dim3(RS_THREADS), 0, ctx->stream, pts, n, model, P.m, t2, state, d_ws + P.off_mask);
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
