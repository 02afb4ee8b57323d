// Robust rigid 3-D motion between paired 3-D points on the GPU: the RANSAC search tests/rigid_restate.py states (DESIGN.md section
// 4.39; pair of a track, hypothesis, inlier tests, refit and plan: vp_rigid_plan.h; point test and stop rule: vp_plane_plan.h; mixer
// and sampler: vp_model_plan.h; the scan and the key reduction: vp_ransac_dev.h).  A call enqueues three launches that compact the
// usable pairs in index order - counts per run of RG_RUN candidates, a scan, the ranked write; no atomic decides a position - then,
// per round of RS_ROUND hypotheses, one scoring launch and one one-block launch that picks the round's best, folds it into the
// running best, applies the stop rule and forms the next round's hypotheses; once the `done` word is set every later launch returns
// at once.  A last launch writes the inlier bytes through the kept indices and adds the sums of the refit.  The number of usable
// pairs stays on the device: grids are sized for the pairs given, and blocks past the usable ones leave.  Counts are integers added
// with integer atomics; only the refit sums depend on the order blocks run in.  This unit is compiled without floating-point
// contraction.
#include "vp_internal.h"
#include "vp_rigid_plan.h"
#include "vp_ransac_dev.h"

// where the candidates come from: two arrays of n points, or n tracks into two images of points
struct rg_source {
    const float* src; const float* dst;      // tracks == 0
    vp_rg_tracks T;                          // tracks != 0
    int n, tracks;
};

// candidate i in index order -> its pair; false when it is not usable
__device__ __forceinline__ bool rg_candidate(const rg_source& G, int i, float p[3], float q[3])
{
    if (i >= G.n) return false;
    if (G.tracks) return vp_rg_track_pair(G.T, i, p, q);
#pragma unroll
    for (int c = 0; c < 3; c++) { p[c] = G.src[(size_t)i * 3 + c]; q[c] = G.dst[(size_t)i * 3 + c]; }
    return vp_pl_usable(p[0], p[1], p[2]) && vp_pl_usable(q[0], q[1], q[2]);
}

// One block per run of RG_RUN candidates, RG_RUN / RG_THREADS passes; in pass p wave v looks at the 64 candidates starting at
// p RG_THREADS + 64 v of the run, so the ballots of (p, v) in that order are the run in index order.  WRITE false: the run's count.
// WRITE true: every usable pair goes to its rank - the run's offset, the counts of the ballots before its own, the set bits below
// its lane - as two float4: p and the original index, q and a zero.
template <bool WRITE>
__global__ __launch_bounds__(RG_THREADS) void k_rg_compact(rg_source G, int32_t* __restrict__ run_count, const int32_t* __restrict__ run_off, float4* __restrict__ pairs)
{
    constexpr int PASSES = RG_RUN / RG_THREADS, WAVES = RG_THREADS / 64;
    __shared__ int s_wc[PASSES * WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int base = blockIdx.x * RG_RUN;
    bool use[PASSES];
    u64 bal[PASSES];
    float4 vp[PASSES], vq[PASSES];
#pragma unroll
    for (int k = 0; k < PASSES; k++) {
        const int i = base + k * RG_THREADS + tid;
        float p[3] = {0.f, 0.f, 0.f}, q[3] = {0.f, 0.f, 0.f};
        use[k] = rg_candidate(G, i, p, q);
        bal[k] = __ballot(use[k]);
        vp[k] = make_float4(p[0], p[1], p[2], __int_as_float(i));
        vq[k] = make_float4(q[0], q[1], q[2], 0.f);
        if (lane == 0) s_wc[k * WAVES + wave] = __popcll(bal[k]);
    }
    __syncthreads();
    if (!WRITE) {
        if (tid == 0) {
            int c = 0;
            for (int k = 0; k < PASSES * WAVES; k++) c += s_wc[k];
            run_count[blockIdx.x] = c;
        }
        return;
    }
    const int off = run_off[blockIdx.x];
#pragma unroll
    for (int k = 0; k < PASSES; k++) {
        if (!use[k]) continue;
        int before = 0;
        for (int m = 0; m < k * WAVES + wave; m++) before += s_wc[m];
        const size_t at = 2 * (size_t)(off + before + __popcll(bal[k] & ((1ull << lane) - 1ull)));
        pairs[at] = vp[k];
        pairs[at + 1] = vq[k];
    }
}

// one block: the exclusive scan of the run counts and their total, the number of usable pairs
__global__ __launch_bounds__(RG_THREADS) void k_rg_scan(const int32_t* __restrict__ run_count, int runs, int32_t* __restrict__ run_off, vp_rg_state* __restrict__ state)
{
    __shared__ int s_sum[RG_THREADS];
    vp_rsd_scan_runs<RG_THREADS>(run_count, runs, run_off, &state->n_usable, s_sum);
}

// One block, one thread per hypothesis of a round.  round >= 0: closes that round - the best count with the lowest index, folded
// into the running best (a later round has to be strictly better), then the stop rule.  Unless the search has ended, forms the
// hypotheses of round + 1 and clears their counts.  round == -1 starts a call; with fewer than three pairs there is no search.
__global__ __launch_bounds__(RG_THREADS) void k_rg_select(const float4* __restrict__ pairs, u32 seed, int max_iters, int round, int rounds,
                                                          const double* __restrict__ qcrit, vp_rg_state* __restrict__ state, int32_t* __restrict__ counts,
                                                          int32_t* __restrict__ valid, double* __restrict__ models)
{
    __shared__ u64 s_key[RG_THREADS];
    __shared__ int s_done;
    const int t = threadIdx.x;
    const int n = state->n_usable;
    if (round < 0) {
        if (t == 0) {
            s_done = n < 3;
            state->done = s_done;
            state->rounds = 0;
            state->best_count = -1;
            state->best_j = -1;
            for (int k = 0; k < RG_MODEL; k++) state->best[k] = 0.0;
            for (int k = 0; k < RG_SUMS; k++) state->sums[k] = 0.0;
        }
    } else {
        if (state->done) return;             // the same word in every thread: all return or none
        const int c = valid[t] ? counts[t] : -1;
        const u64 top = vp_rsd_block_max<RG_THREADS>(s_key, t, ((u64)(c + 1) << 8) | (u64)(RG_THREADS - 1 - t));
        if (t == 0) {
            const int bc = (int)(top >> 8) - 1, bt = RG_THREADS - 1 - (int)(top & 255u);
            int best = state->best_count;
            if (bc > best) {
                best = bc;
                state->best_count = bc;
                state->best_j = round * RS_ROUND + bt;
                for (int k = 0; k < RG_MODEL; k++) state->best[k] = models[bt * RG_MODEL + k];
            }
            state->rounds = round + 1;
            s_done = vp_pl_stop(best, n, qcrit[round]) || round + 1 >= rounds;
            state->done = s_done;
        }
    }
    __syncthreads();
    if (s_done) return;
    const int j = (round + 1) * RS_ROUND + t;
    int32_t s[4];
    double M[RG_MODEL] = {};                 // a thread past max_iters stores zeros
    int ok = 0;
    const float* f = reinterpret_cast<const float*>(pairs);
    if (j < max_iters) ok = vp_rg_hypothesis(f, f + 4, 8, n, seed, (u32)j, s, M);
    valid[t] = ok;
    counts[t] = 0;
    for (int k = 0; k < RG_MODEL; k++) models[t * RG_MODEL + k] = M[k];
}

// grid (RS_ROUND / RG_HYP_PER_BLOCK, chunks of RG_STAGE of the most pairs there can be): a block whose chunk starts past the usable
// pairs leaves; the others stage their chunk (32 KB) and the motions of their hypothesis group in LDS once.  A wave walks the chunk 64
// pairs at a time; a lane forms what the test needs of its pair's destination point once and tests the pair against the wave's
// RG_HYP_PER_BLOCK / 4 hypotheses - a ballot per hypothesis, one integer add per wave and hypothesis at the end.
__global__ __launch_bounds__(RG_THREADS) void k_rg_score(const float4* __restrict__ pairs, vp_rg_metric K, const vp_rg_state* __restrict__ state,
                                                         const int32_t* __restrict__ valid, const double* __restrict__ models, int32_t* __restrict__ counts)
{
    constexpr int WAVES = RG_THREADS / 64, TURNS = RG_HYP_PER_BLOCK / WAVES;
    __shared__ float4 s_p[RG_STAGE];
    __shared__ float4 s_q[RG_STAGE];
    __shared__ double s_motion[RG_HYP_PER_BLOCK * RG_MOTION];
    __shared__ int s_valid[RG_HYP_PER_BLOCK];
    if (state->done) return;
    const int n = state->n_usable;
    const int base = blockIdx.y * RG_STAGE;
    if (base >= n) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cnt = n - base < RG_STAGE ? n - base : RG_STAGE;
    for (int i = tid; i < 2 * cnt; i += RG_THREADS) {
        const float4 v = pairs[2 * (size_t)base + i];
        if (i & 1) s_q[i >> 1] = v;
        else s_p[i >> 1] = v;
    }
    const int h0 = blockIdx.x * RG_HYP_PER_BLOCK;
    if (tid < RG_HYP_PER_BLOCK * RG_MOTION) s_motion[tid] = models[(h0 + tid / RG_MOTION) * RG_MODEL + tid % RG_MOTION];
    if (tid < RG_HYP_PER_BLOCK) s_valid[tid] = valid[h0 + tid];
    __syncthreads();
    int c[TURNS];
#pragma unroll
    for (int k = 0; k < TURNS; k++) c[k] = 0;
    for (int i0 = 0; i0 < cnt; i0 += 64) {
        const int i = i0 + lane;
        const bool live = i < cnt;
        const float4 p = live ? s_p[i] : make_float4(0.f, 0.f, 0.f, 0.f), q = live ? s_q[i] : make_float4(0.f, 0.f, 1.f, 0.f);
        const vp_rg_dst D = vp_rg_dst_side(K, (double)q.x, (double)q.y, (double)q.z);
#pragma unroll
        for (int k = 0; k < TURNS; k++) {
            const int h = wave + k * WAVES;
            bool in = false;
            if (live && s_valid[h]) in = vp_rg_inlier(&s_motion[h * RG_MOTION], K, (double)p.x, (double)p.y, (double)p.z, D);
            c[k] += __popcll(__ballot(in));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < TURNS; k++)
            if (c[k]) atomicAdd(&counts[h0 + wave + k * WAVES], c[k]);
    }
}

// the inlier bytes of the best motion, 1 at the original index of every inlier (the bytes were cleared in front of this launch; inl
// NULL: none wanted), and the seventeen sums of the refit about the best sample's first pair: a wave adds its lanes, lane 0 adds to
// the state
__global__ __launch_bounds__(RG_THREADS) void k_rg_finish(const float4* __restrict__ pairs, vp_rg_metric K, vp_rg_state* __restrict__ state, uint8_t* __restrict__ inl)
{
    const int n = state->n_usable;
    if (state->best_count < 3 || (int)(blockIdx.x * RG_THREADS) >= n) return;
    const int i = blockIdx.x * RG_THREADS + threadIdx.x;
    double M[RG_MODEL];
#pragma unroll
    for (int k = 0; k < RG_MODEL; k++) M[k] = state->best[k];
    double S[RG_SUMS];
#pragma unroll
    for (int k = 0; k < RG_SUMS; k++) S[k] = 0.0;
    bool in = false;
    if (i < n) {
        const float4 p = pairs[2 * (size_t)i], q = pairs[2 * (size_t)i + 1];
        in = vp_rg_inlier(M, K, (double)p.x, (double)p.y, (double)p.z, vp_rg_dst_side(K, (double)q.x, (double)q.y, (double)q.z));
        if (in) {
            const double u[3] = {(double)p.x - M[12], (double)p.y - M[13], (double)p.z - M[14]};
            const double v[3] = {(double)q.x - M[15], (double)q.y - M[16], (double)q.z - M[17]};
#pragma unroll
            for (int c = 0; c < 3; c++) { S[c] = u[c]; S[3 + c] = v[c]; }
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) S[6 + r * 3 + c] = u[r] * v[c];
            S[15] = ((u[0] * u[0]) + (u[1] * u[1])) + (u[2] * u[2]);
            S[16] = ((v[0] * v[0]) + (v[1] * v[1])) + (v[2] * v[2]);
            if (inl) inl[__float_as_int(p.w)] = 1;
        }
    }
    if (!__ballot(in)) return;               // a wave without inliers has nothing to add
#pragma unroll
    for (int k = 0; k < RG_SUMS; k++) {
        const double s = vp_rsd_wave_sum(S[k]);
        if ((threadIdx.x & 63) == 0) atomicAdd(&state->sums[k], s);
    }
}

// src / dst (tracks NULL) or the tracks; every launch of a call, enqueued on the context's stream
int vpk_rg_run(vp_ctx* ctx, const vp_rg_plan& P, const vp_rg_buffers& B, const float* d_src, const float* d_dst, const vp_rg_tracks* tracks, const vp_rg_metric& K,
               int max_iters, u32 seed, uint8_t* d_inl)
{
    rg_source G = {d_src, d_dst, {}, P.n, tracks != nullptr};
    if (tracks) G.T = *tracks;
    float4* pairs = reinterpret_cast<float4*>(B.pairs);
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_rg_compact<false>, dim3(P.runs), dim3(RG_THREADS), 0, ctx->stream, G, B.run_count, B.run_off, pairs);
    }
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_rg_scan, dim3(1), dim3(RG_THREADS), 0, ctx->stream, B.run_count, (int)P.runs, B.run_off, B.state);
    }
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_rg_compact<true>, dim3(P.runs), dim3(RG_THREADS), 0, ctx->stream, G, B.run_count, B.run_off, pairs);
    }
    for (int r = -1; r < P.rounds; r++) {
        if (r >= 0) {
            vp_prof_scope ps(ctx, VPK_OTHER);
            hipLaunchKernelGGL(k_rg_score, dim3(P.score_gx, P.score_gy), dim3(RG_THREADS), 0, ctx->stream, pairs, K, B.state, B.valid, B.models, B.counts);
        }
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_rg_select, dim3(1), dim3(RG_THREADS), 0, ctx->stream, pairs, seed, max_iters, r, P.rounds, B.qcrit, B.state, B.counts, B.valid, B.models);
    }
    if (d_inl) {
        vp_prof_scope ps(ctx, VPK_MEMSET);
        VP_HIP(ctx, hipMemsetAsync(d_inl, 0, (size_t)P.n, ctx->stream));
    }
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_rg_finish, dim3(P.finish_grid), dim3(RG_THREADS), 0, ctx->stream, pairs, K, B.state, d_inl);
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
