// cv2.HoughLines (utils/feature.py:183-213 `find_lines`): OpenCV 4.x HoughLinesStandard with srn == stn == 0, linesMax = INT_MAX.
//
// What is reproduced (imgproc/src/hough.cpp):
//   irho = 1.f / rho; numrho = cvRound((2 (w + h) + 1) / rho) in float; numangle = computeNumangle(min_theta, max_theta, theta) in double;
//   tabSin[n] = (float)(sin((double)ang) * irho), ang accumulated in float from (float)min_theta (made on the host, libm);
//   a nonzero pixel (j, i) votes, for every n, at r = cvRound(j * tabCos[n] + i * tabSin[n]) + (numrho - 1) / 2 into the
//   (numangle + 2) x (numrho + 2) int32 accumulator, cell (n + 1) * (numrho + 2) + r + 1 (two rounded float products, one rounded add);
//   a cell is a line when it is above the threshold, above its left and upper neighbours and not below its right and lower ones;
//   lines are ordered by votes descending, then cell index ascending (hough_cmp_gt, a total order);
//   rho_out = (r - (numrho - 1) * 0.5f) * rho, theta_out = (float)min_theta + n * theta, in float.
// The votes are integer counts, so the order in which the GPU adds them does not change a bit of the result.
//
// Steps (one launch sequence for n equal-shape frames, frame index in grid.y):
//   k_hough_points   nonzero pixels -> packed (x | y << 16) list per frame, one atomic per block of 4096 pixels
//   k_hough_vote     a block takes a slab of angles and a chunk of the points; the slab's accumulator rows are counted in LDS and
//                    the nonzero counts flushed with global atomics (VP_OPT_HOUGH_LDS 0, or rows wider than the LDS budget: every
//                    vote is a global atomic)
//   k_hough_peaks    one thread per cell; peaks appended as 64-bit keys (~votes << 32 | cell), ascending key = cv2's order
//   k_hough_sort_seg one block sorts HS_SEG keys in LDS (bitonic): all of a frame with at most HS_SEG peaks
//   k_hough_merge    above that, sorted runs merged pairwise: a key's place in the merged run is its place in its own run plus the
//                    number of keys of the partner run below it (keys are distinct, so the rank is exact)
//   k_hough_lines    key -> (rho, theta), packed frame after frame, one D2H copy of all lines
#include "vp_internal.h"
#include <cmath>
#include <cstring>
#include <vector>

#define HS_SEG 2048            // keys one block sorts in LDS
#define HV_MINCHUNK 4096       // fewest points a voting block takes (below that the row zeroing and flush outweigh the votes)
#define HV_LDS_BYTES (48 << 10)

// grid (ceil(w * h / 4096), n), 256 threads of 16 pixels each: one atomic per block on the frame's point counter (one per wave was
// a queue of 32 k atomics on one address per 1080p frame)
__global__ __launch_bounds__(256) void k_hough_points(const uint8_t* __restrict__ src, size_t stride, size_t fstride, int w, int h,
                                                      u32* __restrict__ pts, size_t pcap, u32* __restrict__ npts)
{
    __shared__ u32 wsum[4], wbase[4];
    const int f = blockIdx.y;
    const size_t npx = (size_t)w * h;
    const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 16;
    const uint8_t* sf = src + f * fstride;
    u32 bits = 0;
    for (int k = 0; k < 16; k++) {
        const size_t i = i0 + k;
        if (i < npx) {
            const size_t y = i / (unsigned)w, x = i - y * w;
            if (sf[y * stride + x]) bits |= 1u << k;
        }
    }
    const u32 cnt = __popc(bits);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 v = cnt;
    for (int d = 1; d < 64; d <<= 1) {
        const u32 t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const u32 tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        u32 b = tot ? atomicAdd(&npts[f], tot) : 0;
        for (int q = 0; q < 4; q++) { wbase[q] = b; b += wsum[q]; }
    }
    __syncthreads();
    u32 o = wbase[wave] + v - cnt;
    u32* pf = pts + f * pcap;
    while (bits) {
        const int k = __ffs(bits) - 1;
        bits &= bits - 1;
        const size_t i = i0 + k;
        const u32 y = (u32)(i / (unsigned)w), x = (u32)(i - (size_t)y * w);
        pf[o++] = x | (y << 16);
    }
}

// grid (slabs * chunks, n).  lds: rows of the slab's angles (LDS form only).  Votes outside the row (never for r in [-1, numrho])
// go to the global accumulator at the same flat index, as OpenCV's pointer arithmetic would.
template <bool LDS>
__global__ __launch_bounds__(256) void k_hough_vote(const u32* __restrict__ pts, size_t pcap, const u32* __restrict__ npts_arr,
                                                    int* __restrict__ acc, size_t acc_cells, const float* __restrict__ tab_cos,
                                                    const float* __restrict__ tab_sin, int numangle, int numrho, int A, int slabs, int chunks)
{
    extern __shared__ int hv_rows[];
    const int f = blockIdx.y;
    const int slab = blockIdx.x % slabs, c = blockIdx.x / slabs;
    const u32 npts = npts_arr[f];
    if (npts == 0) return;
    const u32 ceff = min((u32)chunks, (npts + HV_MINCHUNK - 1) / HV_MINCHUNK);
    if ((u32)c >= ceff) return;
    const u32 lo = (u32)((u64)npts * c / ceff), hi = (u32)((u64)npts * (c + 1) / ceff);
    const int n0 = slab * A, na = min(A, numangle - n0);
    const int rowlen = numrho + 2, half = (numrho - 1) / 2;
    int* accf = acc + f * acc_cells;
    const u32* pf = pts + f * pcap;
    if (LDS) {
        for (int i = threadIdx.x; i < na * rowlen; i += blockDim.x) hv_rows[i] = 0;
        __syncthreads();
    }
    for (u32 p = lo + threadIdx.x; p < hi; p += blockDim.x) {
        const u32 q = pf[p];
        const float fx = (float)(q & 0xffffu), fy = (float)(q >> 16);
        for (int a = 0; a < na; a++) {
            const int n = n0 + a;
            const float v = __fadd_rn(__fmul_rn(fx, tab_cos[n]), __fmul_rn(fy, tab_sin[n]));
            const int idx = __float2int_rn(v) + half + 1;           // r + 1
            if (LDS && idx >= 0 && idx < rowlen) {
                atomicAdd(&hv_rows[a * rowlen + idx], 1);
            } else {
                const long long g = (long long)(n + 1) * rowlen + idx;
                if (g >= 0 && g < (long long)acc_cells) atomicAdd(&accf[g], 1);
            }
        }
    }
    if (LDS) {
        __syncthreads();
        int* dst = accf + (size_t)(n0 + 1) * rowlen;
        for (int i = threadIdx.x; i < na * rowlen; i += blockDim.x) {
            const int v = hv_rows[i];
            if (v) atomicAdd(&dst[i], v);
        }
    }
}

// grid (ceil(numangle * numrho / 256), n)
__global__ __launch_bounds__(256) void k_hough_peaks(const int* __restrict__ acc, size_t acc_cells, int numangle, int numrho, int threshold,
                                                     u64* __restrict__ keys, size_t kcap, u32* __restrict__ nkeys)
{
    const int f = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool pk = false;
    u64 key = 0;
    if (i < (size_t)numangle * numrho) {
        const int n = (int)(i / (unsigned)numrho), r = (int)(i - (size_t)n * numrho);
        const int rowlen = numrho + 2;
        const int base = (n + 1) * rowlen + r + 1;
        const int* a = acc + f * acc_cells;
        const int v = a[base];
        pk = v > threshold && v > a[base - 1] && v >= a[base + 1] && v > a[base - rowlen] && v >= a[base + rowlen];
        key = ((u64)(~(u32)v) << 32) | (u32)base;
    }
    const u64 m = __ballot(pk);
    if (m == 0) return;
    const int lane = __lane_id();
    const int leader = __ffsll((long long)m) - 1;
    u32 base = 0;
    if (lane == leader) base = atomicAdd(&nkeys[f], (u32)__popcll(m));
    base = __shfl(base, leader);
    const size_t pos = (size_t)base + __popcll(m & ((1ull << lane) - 1ull));
    if (pk && pos < kcap) keys[f * kcap + pos] = key;
}

// grid (segments, n), 1024 threads: sorts keys [s * HS_SEG, min(cnt, (s + 1) * HS_SEG)) of frame blockIdx.y in place
__global__ __launch_bounds__(1024) void k_hough_sort_seg(u64* __restrict__ keys, size_t kcap, const u32* __restrict__ nkeys)
{
    __shared__ u64 s[HS_SEG];
    const int f = blockIdx.y;
    const u32 cnt = nkeys[f];
    const u32 lo = blockIdx.x * HS_SEG;
    if (lo >= cnt) return;
    const u32 len = min((u32)HS_SEG, cnt - lo);
    u64* k = keys + f * kcap + lo;
    for (u32 i = threadIdx.x; i < HS_SEG; i += blockDim.x) s[i] = i < len ? k[i] : ~0ull;
    __syncthreads();
    for (u32 size = 2; size <= HS_SEG; size <<= 1) {
        for (u32 stride = size >> 1; stride > 0; stride >>= 1) {
            for (u32 t = threadIdx.x; t < HS_SEG / 2; t += blockDim.x) {
                const u32 i = 2 * t - (t & (stride - 1));          // first of the pair (bit `stride` clear)
                const u32 j = i + stride;
                const bool up = (i & size) == 0;
                const u64 a = s[i], b = s[j];
                if ((a > b) == up) { s[i] = b; s[j] = a; }
            }
            __syncthreads();
        }
    }
    for (u32 i = threadIdx.x; i < len; i += blockDim.x) k[i] = s[i];
}

// grid (ceil(maxcnt / 256), n): runs of `run` sorted keys in src -> runs of 2 * run in dst
__global__ __launch_bounds__(256) void k_hough_merge(const u64* __restrict__ src, u64* __restrict__ dst, size_t kcap, const u32* __restrict__ nkeys,
                                                     u32 run)
{
    const int f = blockIdx.y;
    const u32 cnt = nkeys[f];
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    const u64* s = src + f * kcap;
    const u64 key = s[i];
    const u32 q = i / run, own = i - q * run;
    const u32 p0 = (q ^ 1u) * run;
    u32 lo = min(p0, cnt), hi = min(p0 + run, cnt);
    const u32 pstart = lo;
    while (lo < hi) {                              // partner keys below `key`
        const u32 mid = (lo + hi) >> 1;
        if (s[mid] < key) lo = mid + 1; else hi = mid;
    }
    dst[f * kcap + (size_t)min(q, q ^ 1u) * run + own + (lo - pstart)] = key;
}

// grid (ceil(max K / 256), n): the first K_f keys of frame f -> lines at out + off[f]
__global__ __launch_bounds__(256) void k_hough_lines(const u64* __restrict__ keys, size_t kcap, const u32* __restrict__ kout,
                                                     const u32* __restrict__ off, int numrho, float rho, float theta, float min_theta,
                                                     float* __restrict__ out)
{
    const int f = blockIdx.y;
    const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= kout[f]) return;
    const u32 base = (u32)keys[f * kcap + k];
    const int rowlen = numrho + 2;
    const int n = (int)(base / (u32)rowlen) - 1;   // cvFloor(idx * (1. / (numrho + 2))) - 1: the same integer for every cell a peak can be in
    const int r = (int)base - (n + 1) * rowlen - 1;
    float* o = out + 2 * ((size_t)off[f] + k);
    o[0] = __fmul_rn(__fsub_rn((float)r, (float)(numrho - 1) * 0.5f), rho);
    o[1] = __fadd_rn(min_theta, __fmul_rn((float)n, theta));
}

int vpk_hough_sort_keys(vp_ctx* ctx, u64* d_k0, u64* d_k1, size_t kcap, const u32* d_nkeys, int n, u32 maxcnt, u64** sorted)
{
    u64* src = d_k0;
    u64* dst = d_k1;
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_hough_sort_seg, dim3((maxcnt + HS_SEG - 1) / HS_SEG, n), dim3(1024), 0, ctx->stream, d_k0, kcap, d_nkeys);
    }
    VP_HIP(ctx, hipGetLastError());
    for (u32 run = HS_SEG; run < maxcnt; run *= 2) {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_hough_merge, dim3((maxcnt + 255) / 256, n), dim3(256), 0, ctx->stream, src, dst, kcap, d_nkeys, run);
        VP_HIP(ctx, hipGetLastError());
        std::swap(src, dst);
    }
    *sorted = src;
    return VP_OK;
}

namespace {
struct hough_geom {
    float rho, theta, irho;
    int numrho, numangle;
    size_t acc_cells, kcap, pcap;
};

int hough_geometry(vp_ctx* ctx, int w, int h, double rho, double theta, double min_theta, double max_theta, hough_geom* g)
{
    if (!(rho > 0) || !(theta > 0) || !std::isfinite(rho) || !std::isfinite(theta) || !std::isfinite(min_theta) || !std::isfinite(max_theta) ||
        max_theta < min_theta)
        return vp_fail(ctx, VP_ERR_INVALID, "hough lines: rho > 0, theta > 0, max_theta >= min_theta");
    g->rho = (float)rho;
    g->theta = (float)theta;
    if (!(g->rho > 0) || !(g->theta > 0)) return vp_fail(ctx, VP_ERR_INVALID, "hough lines: rho / theta vanish as floats");
    g->irho = 1.f / g->rho;
    const int max_rho = w + h, min_rho = -max_rho;
    const float nr = (float)((max_rho - min_rho) + 1) / g->rho;
    const double na = (max_theta - min_theta) / (double)g->theta;
    if (!(nr < (float)(1 << 24)) || !(na < (double)(1 << 24))) return vp_fail(ctx, VP_ERR_UNSUPPORTED, "hough lines: accumulator too large");
    g->numrho = (int)std::nearbyint(nr);           // cvRound: half to even (default rounding mode)
    int numangle = (int)std::floor(na) + 1;
    if (numangle > 1 && std::fabs(M_PI - (numangle - 1) * (double)g->theta) < (double)g->theta / 2) --numangle;
    g->numangle = numangle;
    g->acc_cells = (size_t)(numangle + 2) * (size_t)(g->numrho + 2);
    if (g->acc_cells > ((size_t)1 << 28)) return vp_fail(ctx, VP_ERR_UNSUPPORTED, "hough lines: accumulator above 2^28 cells");
    g->kcap = (size_t)numangle * (size_t)((g->numrho + 1) / 2);    // two neighbours of one row cannot both be peaks
    if (g->kcap == 0) g->kcap = 1;
    g->pcap = (size_t)w * h;
    return VP_OK;
}
}  // namespace

int vp_hough_run(vp_ctx* ctx, const uint8_t* d_src, const uint8_t* h_src, size_t stride, size_t fstride, int n, int w, int h, double rho, double theta, int threshold,
                 double min_theta, double max_theta, float* lines, int max_lines, int* n_lines)
{
    hough_geom g;
    int rc = hough_geometry(ctx, w, h, rho, theta, min_theta, max_theta, &g);
    if (rc != VP_OK) return rc;
    if (g.numrho < 1) {                            // no row of cells: cv2 finds nothing
        for (int f = 0; f < n; f++) n_lines[f] = 0;
        return VP_OK;
    }
    const size_t kout_cap = (size_t)n * std::min((size_t)max_lines, g.kcap);
    vp_ws_frame W;
    float *d_tab, *d_out;
    u32 *d_cnt, *d_kout, *d_pts;
    int* d_acc;
    u64 *d_k0, *d_k1;
    uint8_t* d_img;
    W.want(&d_tab, (size_t)g.numangle * 8);
    W.want(&d_cnt, (size_t)n * 8);                  // points, then peaks, per frame
    W.want(&d_kout, (size_t)n * 8);                 // lines kept, then their offset in the output, per frame
    W.want(&d_pts, g.pcap * 4 * n);
    W.want(&d_acc, g.acc_cells * 4 * n);
    W.want(&d_k0, g.kcap * 8 * n);
    W.want(&d_k1, g.kcap * 8 * n);
    W.want(&d_out, std::max(kout_cap, (size_t)1) * 8);
    if (h_src) W.want(&d_img, (size_t)w * h);
    rc = vp_ws_commit(ctx, W, "hough workspace");
    if (rc != VP_OK) return rc;
    if (h_src) {
        VP_HIP(ctx, hipMemcpyAsync(d_img, h_src, (size_t)w * h, hipMemcpyHostToDevice, ctx->stream));
        d_src = d_img;
    }
    u32* d_npts = d_cnt;
    u32* d_nk = d_cnt + n;
    u32* d_off = d_kout + n;

    // trig tables, as createTrigTable makes them
    std::vector<float> tab((size_t)g.numangle * 2);
    float ang = (float)min_theta;
    for (int k = 0; k < g.numangle; ang += g.theta, k++) {
        tab[k] = (float)(std::cos((double)ang) * g.irho);
        tab[g.numangle + k] = (float)(std::sin((double)ang) * g.irho);
    }
    uint8_t* hs = (uint8_t*)vp_hstage(ctx, std::max(tab.size() * 4, (size_t)n * 8));
    if (!hs) return vp_fail(ctx, VP_ERR_NOMEM, "pinned staging");
    VP_HIP(ctx, hipStreamSynchronize(ctx->stream));     // the staging buffer may still be the source of an earlier copy
    memcpy(hs, tab.data(), tab.size() * 4);
    VP_HIP(ctx, hipMemcpyAsync(d_tab, hs, tab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    VP_HIP(ctx, hipMemsetAsync(d_cnt, 0, (size_t)n * 8, ctx->stream));
    VP_HIP(ctx, hipMemsetAsync(d_acc, 0, g.acc_cells * 4 * n, ctx->stream));

    const size_t npx = (size_t)w * h;
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_hough_points, dim3((unsigned)((npx + 4095) / 4096), n), dim3(256), 0, ctx->stream, d_src, stride, fstride, w, h, d_pts,
                           g.pcap, d_npts);
    }
    VP_HIP(ctx, hipGetLastError());

    const size_t rowbytes = (size_t)(g.numrho + 2) * 4;
    const bool lds = ctx->opt.v[VP_OPT_HOUGH_LDS] && rowbytes <= HV_LDS_BYTES;
    const int A = lds ? (int)std::min<size_t>(16, HV_LDS_BYTES / rowbytes) : 16;
    const int slabs = (g.numangle + A - 1) / A;
    const int cu = ctx->num_cu > 0 ? ctx->num_cu : 256;
    const size_t want = (size_t)8 * cu;                                     // blocks to cover the chip several times over
    size_t chunks = std::max<size_t>(1, (want + (size_t)slabs * n - 1) / ((size_t)slabs * n));
    chunks = std::min(chunks, std::max<size_t>(1, (g.pcap + HV_MINCHUNK - 1) / HV_MINCHUNK));
    if ((size_t)slabs * chunks > 0x7fffffffu) return vp_fail(ctx, VP_ERR_UNSUPPORTED, "hough lines: voting grid");
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        if (lds)
            hipLaunchKernelGGL(k_hough_vote<true>, dim3((unsigned)(slabs * chunks), n), dim3(256), (size_t)A * rowbytes, ctx->stream, d_pts, g.pcap,
                               d_npts, d_acc, g.acc_cells, d_tab, d_tab + g.numangle, g.numangle, g.numrho, A, slabs, (int)chunks);
        else
            hipLaunchKernelGGL(k_hough_vote<false>, dim3((unsigned)(slabs * chunks), n), dim3(256), 0, ctx->stream, d_pts, g.pcap, d_npts, d_acc,
                               g.acc_cells, d_tab, d_tab + g.numangle, g.numangle, g.numrho, A, slabs, (int)chunks);
    }
    VP_HIP(ctx, hipGetLastError());
    const size_t ncell = (size_t)g.numangle * g.numrho;
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_hough_peaks, dim3((unsigned)((ncell + 255) / 256), n), dim3(256), 0, ctx->stream, d_acc, g.acc_cells, g.numangle,
                           g.numrho, threshold, d_k0, g.kcap, d_nk);
    }
    VP_HIP(ctx, hipGetLastError());
    // the peak counts size the sort and the copy-out
    VP_HIP(ctx, hipMemcpyAsync(hs, d_nk, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    VP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<u32> cnt(n), kout(n), off(n);
    memcpy(cnt.data(), hs, (size_t)n * 4);
    u32 maxcnt = 0, maxk = 0;
    size_t total = 0;
    for (int f = 0; f < n; f++) {
        if ((size_t)cnt[f] > g.kcap) return vp_fail(ctx, VP_ERR_HIP, "hough lines: peak count above its bound");
        n_lines[f] = (int)cnt[f];
        kout[f] = std::min(cnt[f], (u32)max_lines);
        off[f] = (u32)total;
        total += kout[f];
        maxcnt = std::max(maxcnt, cnt[f]);
        maxk = std::max(maxk, kout[f]);
    }
    if (total == 0) return VP_OK;
    memcpy(hs, kout.data(), (size_t)n * 4);
    memcpy(hs + (size_t)n * 4, off.data(), (size_t)n * 4);
    VP_HIP(ctx, hipMemcpyAsync(d_kout, hs, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    u64* src = nullptr;
    rc = vpk_hough_sort_keys(ctx, d_k0, d_k1, g.kcap, d_nk, n, maxcnt, &src);
    if (rc != VP_OK) return rc;
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_hough_lines, dim3((maxk + 255) / 256, n), dim3(256), 0, ctx->stream, src, g.kcap, d_kout, d_off, g.numrho, g.rho,
                           g.theta, (float)min_theta, d_out);
    }
    VP_HIP(ctx, hipGetLastError());
    float* hl = (float*)vp_hstage(ctx, total * 8);
    if (!hl) return vp_fail(ctx, VP_ERR_NOMEM, "pinned staging");
    VP_HIP(ctx, hipMemcpyAsync(hl, d_out, total * 8, hipMemcpyDeviceToHost, ctx->stream));
    VP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int f = 0; f < n; f++)
        if (kout[f]) memcpy(lines + (size_t)f * max_lines * 2, hl + (size_t)off[f] * 2, (size_t)kout[f] * 8);
    return VP_OK;
}
