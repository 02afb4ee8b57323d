// Device bodies the RANSAC units share (vp_model.hip, vp_plane.hip, vp_rigid.hip): the key reduction of the one-block select launch
// and the one-block scan of the compaction's run counts.  Kernel units only; every function is called by all threads of the block.
#pragma once
#include "vp_internal.h"

// The largest key of the block, valid in thread 0.  A select block packs (count + 1) << 8 | (THREADS - 1 - t) into `mine`, so the
// largest key is the best count and, among equals, the lowest thread.
template <int THREADS, typename KEY>
__device__ __forceinline__ KEY vp_rsd_block_max(KEY* s_key, int t, KEY mine)
{
    s_key[t] = mine;
    __syncthreads();
    for (int w = THREADS / 2; w >= 1; w >>= 1) {
        if (t < w && s_key[t + w] > s_key[t]) s_key[t] = s_key[t + w];
        __syncthreads();
    }
    return s_key[0];
}

// run_off = the exclusive scan of run_count[0 .. runs), *total = their sum (written by thread 0); s_sum: THREADS ints of LDS
template <int THREADS>
__device__ __forceinline__ void vp_rsd_scan_runs(const int32_t* __restrict__ run_count, int runs, int32_t* __restrict__ run_off, int32_t* __restrict__ total, int* s_sum)
{
    const int t = threadIdx.x, per = (runs + THREADS - 1) / THREADS;
    const int lo = t * per < runs ? t * per : runs, hi = lo + per < runs ? lo + per : runs;
    int c = 0;
    for (int i = lo; i < hi; i++) c += run_count[i];
    s_sum[t] = c;
    __syncthreads();
    if (t == 0) {
        int acc = 0;
        for (int k = 0; k < THREADS; k++) { const int v = s_sum[k]; s_sum[k] = acc; acc += v; }
        *total = acc;
    }
    __syncthreads();
    int acc = s_sum[t];
    for (int i = lo; i < hi; i++) { run_off[i] = acc; acc += run_count[i]; }
}

// the sum of a double over the 64 lanes of a wave, valid in lane 0
__device__ __forceinline__ double vp_rsd_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
