// Robust plane fitting to the 3-D points of an image on the GPU: the RANSAC search tests/plane_restate.py states (DESIGN.md section
// 4.38; point test, hypothesis, inlier test, stop rule and plan: vp_plane_plan.h; mixer and sampler: vp_model_plan.h).  A call
// enqueues three launches that compact the usable points of the box in raster order - counts per run of PL_RUN candidates, a scan,
// the ranked write; no atomic decides a position - then, per round of RS_ROUND hypotheses, one scoring launch and one one-block launch
// that picks the round's best, folds it into the running best, applies the stop rule and forms the next round's hypotheses; once the
// `done` word is set every later launch returns at once.  A last launch writes the inlier bytes through the pixel indices and adds
// the sums of the refit.  The number of points stays on the device: grids are sized for the box, and blocks past the points leave.
// Counts are integers added with integer atomics; only the refit sums depend on the order blocks run in.  This unit is compiled
// without floating-point contraction.
#include "vp_internal.h"
#include "vp_plane_plan.h"
#include "vp_ransac_dev.h"

struct pl_image {
    const float* xyz; size_t xstride;        // bytes
    const uint8_t* mask; size_t mstride;     // mask NULL: every pixel of the box is a candidate
    int w;
    vp_pl_box box;
    int ncand;
};

// candidate q of the box in raster order -> its pixel index and point; false when it is not usable
__device__ __forceinline__ bool pl_candidate(const pl_image& I, int q, int* index, float* x, float* y, float* z)
{
    if (q >= I.ncand) return false;
    const int yy = q / I.box.rw, py = I.box.y0 + yy, px = I.box.x0 + (q - yy * I.box.rw);
    if (I.mask && !I.mask[(size_t)py * I.mstride + px]) return false;
    const float* p = reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(I.xyz) + (size_t)py * I.xstride) + 3 * (size_t)px;
    *x = p[0]; *y = p[1]; *z = p[2];
    *index = py * I.w + px;
    return vp_pl_usable(*x, *y, *z);
}

// One block per run of PL_RUN candidates, PL_RUN / PL_THREADS passes; in pass p wave v looks at the 64 candidates starting at
// p PL_THREADS + 64 v of the run, so the ballots of (p, v) in that order are the run in raster order.  WRITE false: the run's count.
// WRITE true: every usable candidate goes to its rank - the run's offset, the counts of the ballots before its own, the set bits
// below its lane.
template <bool WRITE>
__global__ __launch_bounds__(PL_THREADS) void k_pl_compact(pl_image I, int32_t* __restrict__ run_count, const int32_t* __restrict__ run_off, float4* __restrict__ pts)
{
    constexpr int PASSES = PL_RUN / PL_THREADS, WAVES = PL_THREADS / 64;
    __shared__ int s_wc[PASSES * WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int base = blockIdx.x * PL_RUN;
    bool use[PASSES];
    u64 bal[PASSES];
    float4 v[PASSES];
#pragma unroll
    for (int p = 0; p < PASSES; p++) {
        int index = 0;
        float x = 0.f, y = 0.f, z = 0.f;
        use[p] = pl_candidate(I, base + p * PL_THREADS + tid, &index, &x, &y, &z);
        bal[p] = __ballot(use[p]);
        v[p] = make_float4(x, y, z, __int_as_float(index));
        if (lane == 0) s_wc[p * WAVES + wave] = __popcll(bal[p]);
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
    for (int p = 0; p < PASSES; p++) {
        if (!use[p]) continue;
        int before = 0;
        for (int k = 0; k < p * WAVES + wave; k++) before += s_wc[k];
        pts[off + before + __popcll(bal[p] & ((1ull << lane) - 1ull))] = v[p];
    }
}

// one block: the exclusive scan of the run counts and their total, the number of points
__global__ __launch_bounds__(PL_THREADS) void k_pl_scan(const int32_t* __restrict__ run_count, int runs, int32_t* __restrict__ run_off, vp_pl_state* __restrict__ state)
{
    __shared__ int s_sum[PL_THREADS];
    vp_rsd_scan_runs<PL_THREADS>(run_count, runs, run_off, &state->n_usable, s_sum);
}

// One block, one thread per hypothesis of a round.  round >= 0: closes that round - the best count with the lowest index, folded
// into the running best (a later round has to be strictly better), then the stop rule.  Unless the search has ended, forms the
// hypotheses of round + 1 and clears their counts.  round == -1 starts a call; with fewer than three points there is no search.
__global__ __launch_bounds__(PL_THREADS) void k_pl_select(const float4* __restrict__ pts, int metric, u32 seed, int max_iters, int round, int rounds,
                                                          const double* __restrict__ qcrit, vp_pl_state* __restrict__ state, int32_t* __restrict__ counts,
                                                          int32_t* __restrict__ valid, double* __restrict__ models)
{
    __shared__ u64 s_key[PL_THREADS];
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
            for (int k = 0; k < PL_MODEL; k++) state->best[k] = 0.0;
            for (int k = 0; k < PL_SUMS; k++) state->sums[k] = 0.0;
        }
    } else {
        if (state->done) return;             // the same word in every thread: all return or none
        const int c = valid[t] ? counts[t] : -1;
        const u64 top = vp_rsd_block_max<PL_THREADS>(s_key, t, ((u64)(c + 1) << 8) | (u64)(PL_THREADS - 1 - t));
        if (t == 0) {
            const int bc = (int)(top >> 8) - 1, bt = PL_THREADS - 1 - (int)(top & 255u);
            int best = state->best_count;
            if (bc > best) {
                best = bc;
                state->best_count = bc;
                state->best_j = round * RS_ROUND + bt;
                for (int k = 0; k < PL_MODEL; k++) state->best[k] = models[bt * PL_MODEL + k];
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
    double M[PL_MODEL];
    int ok = 0;
    if (j < max_iters) ok = vp_pl_hypothesis(reinterpret_cast<const float*>(pts), n, metric, seed, (u32)j, s, M);
    valid[t] = ok;
    counts[t] = 0;
    for (int k = 0; k < PL_MODEL; k++) models[t * PL_MODEL + k] = M[k];
}

// grid (RS_ROUND / PL_HYP_PER_BLOCK, chunks of PL_STAGE of the most points there can be): a block whose chunk starts past the points
// leaves; the others stage their chunk in LDS once, then each of the four waves tests it against every fourth hypothesis of the
// block's group - a ballot per 64 points, one integer add per wave and hypothesis
__global__ __launch_bounds__(PL_THREADS) void k_pl_score(const float4* __restrict__ pts, int metric, double t2, const vp_pl_state* __restrict__ state,
                                                         const int32_t* __restrict__ valid, const double* __restrict__ models, int32_t* __restrict__ counts)
{
    __shared__ float4 s_pts[PL_STAGE];
    if (state->done) return;
    const int n = state->n_usable;
    const int base = blockIdx.y * PL_STAGE;
    if (base >= n) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cnt = n - base < PL_STAGE ? n - base : PL_STAGE;
    for (int i = tid; i < cnt; i += PL_THREADS) s_pts[i] = pts[base + i];
    __syncthreads();
    const int h0 = blockIdx.x * PL_HYP_PER_BLOCK;
    for (int h = h0 + wave; h < h0 + PL_HYP_PER_BLOCK; h += PL_THREADS / 64) {
        if (!valid[h]) continue;
        double P[4];
#pragma unroll
        for (int k = 0; k < 4; k++) P[k] = models[h * PL_MODEL + k];
        const double lim = vp_pl_limit(P, metric, t2);
        int c = 0;
        for (int i0 = 0; i0 < cnt; i0 += 64) {
            const int i = i0 + lane;
            bool in = false;
            if (i < cnt) {
                const float4 p = s_pts[i];
                in = vp_pl_inlier(P, lim, (double)p.x, (double)p.y, (double)p.z);
            }
            c += __popcll(__ballot(in));
        }
        if (lane == 0 && c) atomicAdd(&counts[h], c);
    }
}

// the inlier bytes of the best plane, 255 at the pixel of every inlier (the image was cleared in front of this launch; inl NULL: none
// wanted), and the nine sums of the refit about the best sample's first point: a wave adds its lanes, lane 0 adds to the state
__global__ __launch_bounds__(PL_THREADS) void k_pl_finish(const float4* __restrict__ pts, int metric, double t2, int w, vp_pl_state* __restrict__ state,
                                                          uint8_t* __restrict__ inl, size_t istride)
{
    const int n = state->n_usable;
    if (state->best_count < 3 || (int)(blockIdx.x * PL_THREADS) >= n) return;
    const int i = blockIdx.x * PL_THREADS + threadIdx.x;
    double P[4], p0[3];
#pragma unroll
    for (int k = 0; k < 4; k++) P[k] = state->best[k];
#pragma unroll
    for (int k = 0; k < 3; k++) p0[k] = state->best[4 + k];
    const double lim = vp_pl_limit(P, metric, t2);
    double S[PL_SUMS];
#pragma unroll
    for (int k = 0; k < PL_SUMS; k++) S[k] = 0.0;
    bool in = false;
    if (i < n) {
        const float4 p = pts[i];
        in = vp_pl_inlier(P, lim, (double)p.x, (double)p.y, (double)p.z);
        if (in) {
            const double u = (double)p.x - p0[0], v = (double)p.y - p0[1], q = (double)p.z - p0[2];
            S[0] = u; S[1] = v; S[2] = q;
            S[3] = u * u; S[4] = u * v; S[5] = u * q;
            S[6] = v * v; S[7] = v * q; S[8] = q * q;
            if (inl) {
                const int index = __float_as_int(p.w), y = index / w;
                inl[(size_t)y * istride + (index - y * w)] = 255;
            }
        }
    }
    if (!__ballot(in)) return;               // a wave without inliers has nothing to add
#pragma unroll
    for (int k = 0; k < PL_SUMS; k++) {
        const double s = vp_rsd_wave_sum(S[k]);
        if ((threadIdx.x & 63) == 0) atomicAdd(&state->sums[k], s);
    }
}

int vpk_pl_run(vp_ctx* ctx, const vp_pl_plan& P, const vp_pl_buffers& B, const float* d_xyz, size_t xstride, int w, int h, const uint8_t* d_mask, size_t mstride,
               int metric, double t2, int max_iters, u32 seed, uint8_t* d_inl, size_t istride)
{
    const pl_image I = {d_xyz, xstride, d_mask, mstride, w, P.box, P.ncand};
    float4* pts = reinterpret_cast<float4*>(B.pts);
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_pl_compact<false>, dim3(P.runs), dim3(PL_THREADS), 0, ctx->stream, I, B.run_count, B.run_off, pts);
    }
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_pl_scan, dim3(1), dim3(PL_THREADS), 0, ctx->stream, B.run_count, (int)P.runs, B.run_off, B.state);
    }
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_pl_compact<true>, dim3(P.runs), dim3(PL_THREADS), 0, ctx->stream, I, B.run_count, B.run_off, pts);
    }
    for (int r = -1; r < P.rounds; r++) {
        if (r >= 0) {
            vp_prof_scope ps(ctx, VPK_OTHER);
            hipLaunchKernelGGL(k_pl_score, dim3(P.score_gx, P.score_gy), dim3(PL_THREADS), 0, ctx->stream, pts, metric, t2, B.state, B.valid, B.models, B.counts);
        }
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_pl_select, dim3(1), dim3(PL_THREADS), 0, ctx->stream, pts, metric, seed, max_iters, r, P.rounds, B.qcrit, B.state, B.counts, B.valid,
                           B.models);
    }
    if (d_inl) {
        vp_prof_scope ps(ctx, VPK_MEMSET);
        VP_HIP(ctx, hipMemset2DAsync(d_inl, istride, 0, (size_t)w, (size_t)h, ctx->stream));
    }
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_pl_finish, dim3(P.finish_grid), dim3(PL_THREADS), 0, ctx->stream, pts, metric, t2, w, B.state, d_inl, istride);
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
