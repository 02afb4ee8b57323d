// Feature kernels: FAST-9 corners, the steered 256-bit binary descriptor and the brute-force Hamming matcher (DESIGN.md section 4.31;
// every host decision: vp_features_plan.h; the statement: tests/features_restate.py), and the same detector and descriptor over all
// levels of a scale pyramid at once (section 4.32; tests/pyr_features_restate.py).  All integer arithmetic.
#include "vp_internal.h"
#include "vp_features_plan.h"

namespace {

// ---- FAST-9 ------------------------------------------------------------------------------------------------------------------------
// M of the centre v over the ring r[0..15]: the largest t' + 1 such that nine contiguous ring pixels are all darker than v - t' or all
// brighter than v + t'.  min over nine contiguous entries by doubling: windows of 2, 4, 8, then one more.
__device__ __forceinline__ int fast_m(int v, const int (&r)[16])
{
    int d[16], lo2[16], hi2[16], lo4[16], hi4[16];
#pragma unroll
    for (int j = 0; j < 16; j++) d[j] = v - r[j];
#pragma unroll
    for (int j = 0; j < 16; j++) { lo2[j] = min(d[j], d[(j + 1) & 15]); hi2[j] = max(d[j], d[(j + 1) & 15]); }
#pragma unroll
    for (int j = 0; j < 16; j++) { lo4[j] = min(lo2[j], lo2[(j + 2) & 15]); hi4[j] = max(hi2[j], hi2[(j + 2) & 15]); }
    int best = -256;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const int lo9 = min(min(lo4[j], lo4[(j + 4) & 15]), d[(j + 8) & 15]);     // all nine darker than v by at least lo9
        const int hi9 = max(max(hi4[j], hi4[(j + 4) & 15]), d[(j + 8) & 15]);     // all nine brighter than v by at least -hi9
        best = max(best, max(lo9, -hi9));
    }
    return best;
}

// Tile (bx, by) of an image by one block of 256 lanes, four pixels of the FT_TW x FT_TH tile each; tile: the block's LDS.
// score[y w + x] = M where M > threshold and the pixel is a candidate (3 <= x <= w - 4, 3 <= y <= h - 4), else 0.  The staged
// coordinates are clamped into the image: what a clamp changes is read by non-candidates only.
__device__ __forceinline__ void fast_score_tile(const uint8_t* __restrict__ src, size_t stride, int w, int h, int threshold, uint8_t* __restrict__ score, int bx, int by,
                                                uint8_t* tile)
{
    const int x0 = bx * FT_TW, y0 = by * FT_TH;
    constexpr int SW = FT_TW + 2 * FT_FAST_R, SH = FT_TH + 2 * FT_FAST_R;
    for (int i = threadIdx.x; i < SW * SH; i += 256) {
        const int ty = i / SW, tx = i - ty * SW;
        const int gx = min(max(x0 + tx - FT_FAST_R, 0), w - 1), gy = min(max(y0 + ty - FT_FAST_R, 0), h - 1);
        tile[ty * FT_LDS_PITCH + tx] = src[(size_t)gy * stride + gx];
    }
    __syncthreads();
    constexpr int RX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
    constexpr int RY[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
    const int tx = threadIdx.x & (FT_TW - 1), x = x0 + tx;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int ty = (threadIdx.x >> 6) + 4 * q, y = y0 + ty;
        if (x >= w || y >= h) continue;
        int m = 0;
        if (x >= FT_FAST_R && x <= w - 1 - FT_FAST_R && y >= FT_FAST_R && y <= h - 1 - FT_FAST_R) {
            const uint8_t* c = tile + (ty + FT_FAST_R) * FT_LDS_PITCH + tx + FT_FAST_R;
            int r[16];
#pragma unroll
            for (int j = 0; j < 16; j++) r[j] = c[RY[j] * FT_LDS_PITCH + RX[j]];
            const int M = fast_m(c[0], r);
            m = M > threshold ? M : 0;
        }
        score[(size_t)y * w + x] = (uint8_t)m;
    }
}

// grid (tiles_x, tiles_y)
__global__ __launch_bounds__(256) void k_fast_score(const uint8_t* __restrict__ src, size_t stride, int w, int h, int threshold, uint8_t* __restrict__ score)
{
    __shared__ uint8_t tile[(FT_TH + 2 * FT_FAST_R) * FT_LDS_PITCH];
    fast_score_tile(src, stride, w, h, threshold, score, blockIdx.x, blockIdx.y, tile);
}

// grid sel_blocks, FT_SEL_BLOCK lanes, one pixel each in raster order.  keep[i] = score[i] where the corner is kept, else 0;
// cnt[i / 64] = kept corners of that wave.  A corner (score[i] > 0) is never on the image's outermost three rows and columns, so its
// eight neighbours exist.
__global__ __launch_bounds__(FT_SEL_BLOCK) void k_fast_count(const uint8_t* __restrict__ score, int w, size_t npx, int nonmax, uint8_t* __restrict__ keep,
                                                             u32* __restrict__ cnt)
{
    const size_t i = (size_t)blockIdx.x * FT_SEL_BLOCK + threadIdx.x;
    int kv = 0;
    if (i < npx) {
        const int m = score[i];
        if (m) {
            bool k = true;
            if (nonmax) {
#pragma unroll
                for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                    for (int dx = -1; dx <= 1; dx++) {
                        if (!dx && !dy) continue;
                        const int n = score[i + (ptrdiff_t)dy * w + dx];
                        if (!(m - 1 > (n ? n - 1 : 0))) k = false;
                    }
            }
            if (k) kv = m;
        }
        keep[i] = (uint8_t)kv;
    }
    const u64 b = __ballot(kv != 0);
    if ((threadIdx.x & 63) == 0 && i < npx) cnt[i / FT_CHUNK] = (u32)__popcll(b);
}

// one block of FT_SCAN_LANES lanes: cnt[0 .. chunks) becomes its exclusive prefix sum, cnt[chunks] the total
__global__ __launch_bounds__(FT_SCAN_LANES) void k_fast_scan(u32* __restrict__ cnt, size_t chunks, size_t per)
{
    __shared__ u32 wsum[FT_SCAN_LANES / 64];
    const size_t b = (size_t)threadIdx.x * per, e = b + per < chunks ? b + per : chunks;
    u32 s = 0;
    for (size_t i = b; i < e; i++) s += cnt[i];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 inc = s;
    for (int off = 1; off < 64; off <<= 1) {
        const u32 o = (u32)__shfl_up((int)inc, off);
        if (lane >= off) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    u32 before = 0;
    for (int q = 0; q < wave; q++) before += wsum[q];
    u32 run = before + inc - s;
    for (size_t i = b; i < e; i++) {
        const u32 c = cnt[i];
        cnt[i] = run;
        run += c;
    }
    if (threadIdx.x == FT_SCAN_LANES - 1) cnt[chunks] = before + inc;
}

// grid sel_blocks, FT_SEL_BLOCK lanes: kept corner number offs[i / 64] + (kept corners of lower lanes) goes to that slot when it is below cap
__global__ __launch_bounds__(FT_SEL_BLOCK) void k_fast_write(const uint8_t* __restrict__ keep, int w, size_t npx, const u32* __restrict__ offs, int nonmax,
                                                             int32_t* __restrict__ xy, int32_t* __restrict__ val, size_t cap)
{
    const size_t i = (size_t)blockIdx.x * FT_SEL_BLOCK + threadIdx.x;
    const int kv = i < npx ? keep[i] : 0;
    const u64 b = __ballot(kv != 0);
    if (kv) {
        const int lane = threadIdx.x & 63;
        const size_t pos = (size_t)offs[i / FT_CHUNK] + __popcll(b & ((1ull << lane) - 1ull));
        if (pos < cap) {
            const int y = (int)(i / (unsigned)w), x = (int)(i - (size_t)y * w);
            xy[2 * pos] = x;
            xy[2 * pos + 1] = y;
            val[pos] = nonmax ? kv - 1 : 0;
        }
    }
}

// ---- the steered descriptor --------------------------------------------------------------------------------------------------------
struct ft_trig { int32_t c[FT_BINS], s[FT_BINS]; };

// One wave describes the pixel (px, py), at least FT_DESC_BORDER from every border: the orientation bin from src (rows of stride bytes),
// the 256 bits from blur (packed rows of w bytes) into desc[0 .. 4).  Returns the bin; lane 0 writes.
__device__ __forceinline__ int describe_pixel(const uint8_t* __restrict__ src, size_t stride, const uint8_t* __restrict__ blur, int w, int px, int py, int lane,
                                              const int8_t* __restrict__ pattern, const ft_trig& T, u64* __restrict__ desc)
{
    int m10 = 0, m01 = 0;
    for (int i = lane; i < FT_DISC_SIDE * FT_DISC_SIDE; i += 64) {
        const int dy = i / FT_DISC_SIDE - FT_DESC_BORDER, dx = i % FT_DISC_SIDE - FT_DESC_BORDER;
        if (dx * dx + dy * dy <= FT_DISC_R2) {
            const int v = src[(size_t)(py + dy) * stride + (px + dx)];
            m10 += dx * v;
            m01 += dy * v;
        }
    }
    for (int off = 32; off; off >>= 1) {
        m10 += __shfl_xor(m10, off);
        m01 += __shfl_xor(m01, off);
    }
    int kb = 0;
    long long best = (long long)m10 * T.c[0] + (long long)m01 * T.s[0];
    for (int k = 1; k < FT_BINS; k++) {
        const long long sc = (long long)m10 * T.c[k] + (long long)m01 * T.s[k];
        if (sc > best) { best = sc; kb = k; }
    }
    const char4* pat = reinterpret_cast<const char4*>(pattern + (size_t)kb * FT_PAIRS * 4);
    const uint8_t* c = blur + (size_t)py * w + px;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const char4 q = pat[64 * j + lane];
        const int a = c[(ptrdiff_t)q.y * w + q.x], b = c[(ptrdiff_t)q.w * w + q.z];
        const u64 word = __ballot(a < b);
        if (lane == 0) desc[j] = word;
    }
    return kb;
}

// grid ceil(n / FT_DESC_WAVES), FT_DESC_WAVES waves: one wave per point, no LDS and no barrier.  src: rows of stride bytes; blur: packed.
// Every read of an admitted point lies within 15 of its pixel, which is at least 15 from every border.
__global__ __launch_bounds__(64 * FT_DESC_WAVES) void k_describe(const uint8_t* __restrict__ src, size_t stride, const uint8_t* __restrict__ blur, int w, int h,
                                                                 const float* __restrict__ pts, int n, const int8_t* __restrict__ pattern, ft_trig T,
                                                                 u64* __restrict__ desc, uint8_t* __restrict__ bin, uint8_t* __restrict__ status)
{
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * FT_DESC_WAVES + (threadIdx.x >> 6);
    if (p >= n) return;
    const float fx = pts[2 * (size_t)p], fy = pts[2 * (size_t)p + 1];
    const double rx = floor((double)fx + 0.5), ry = floor((double)fy + 0.5);
    const bool ok = isfinite(fx) && isfinite(fy) && rx >= FT_DESC_BORDER && rx <= w - 1 - FT_DESC_BORDER && ry >= FT_DESC_BORDER && ry <= h - 1 - FT_DESC_BORDER;
    if (!ok) {
        if (lane < 4) desc[4 * (size_t)p + lane] = 0;
        if (lane == 0) { bin[p] = 0; status[p] = 0; }
        return;
    }
    const int kb = describe_pixel(src, stride, blur, w, (int)rx, (int)ry, lane, pattern, T, desc + 4 * (size_t)p);
    if (lane == 0) { bin[p] = (uint8_t)kb; status[p] = 1; }
}

// ---- the scale pyramid: every level in each launch ----------------------------------------------------------
// The levels lie one after the other in every per-pixel region (vp_pyr_table, vp_features_plan.h); a block or a wave finds its level
// from the table, which is passed by value, so no launch count depends on the number of levels.
__device__ __forceinline__ int pyr_level_of_px(const vp_pyr_table& T, u32 pos)
{
    int l = 0;
    for (int k = 1; k < FT_PYR_MAX_LEVELS; k++)
        if (k < T.n_levels && pos >= T.L[k].off) l = k;
    return l;
}

// grid T.total_tiles, 256 lanes: the score map of every level, as k_fast_score makes one
__global__ __launch_bounds__(256) void k_pyr_score(const uint8_t* __restrict__ img, vp_pyr_table T, int threshold, uint8_t* __restrict__ score)
{
    __shared__ uint8_t tile[(FT_TH + 2 * FT_FAST_R) * FT_LDS_PITCH];
    int l = 0;
    for (int k = 1; k < FT_PYR_MAX_LEVELS; k++)
        if (k < T.n_levels && blockIdx.x >= T.L[k].tile_begin) l = k;
    const vp_pyr_level L = T.L[l];
    const u32 t = blockIdx.x - L.tile_begin;
    fast_score_tile(img + L.off, (size_t)L.w, L.w, L.h, threshold, score + L.off, (int)(t % L.tiles_x), (int)(t / L.tiles_x), tile);
}

// grid T.total_px / FT_SEL_BLOCK, FT_SEL_BLOCK lanes, one pixel each, the block inside one level.  keep[pos] = score where the pixel
// can be described (15 from every border) and is strictly above its eight neighbours in the level's full score map, else 0 (the
// padding behind a level too).  hist[level][v] counts the kept scores: LDS counters, then one integer add per bin that is not empty.
__global__ __launch_bounds__(FT_SEL_BLOCK) void k_pyr_suppress(const uint8_t* __restrict__ score, vp_pyr_table T, uint8_t* __restrict__ keep, u32* __restrict__ hist)
{
    __shared__ u32 bins[256];
    const u32 pos = blockIdx.x * FT_SEL_BLOCK + threadIdx.x;
    const int l = pyr_level_of_px(T, blockIdx.x * FT_SEL_BLOCK);
    const vp_pyr_level L = T.L[l];
    bins[threadIdx.x] = 0;
    __syncthreads();
    const u32 i = pos - L.off;
    int kv = 0;
    if (i < (u32)L.w * (u32)L.h) {
        const int y = (int)(i / (u32)L.w), x = (int)(i - (u32)y * (u32)L.w);
        if (x >= FT_DESC_BORDER && x <= L.w - 1 - FT_DESC_BORDER && y >= FT_DESC_BORDER && y <= L.h - 1 - FT_DESC_BORDER) {
            const uint8_t* s = score + pos;
            const int m = s[0];
            if (m) {
                bool k = true;
#pragma unroll
                for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                    for (int dx = -1; dx <= 1; dx++) {
                        if (!dx && !dy) continue;
                        const int n = s[(ptrdiff_t)dy * L.w + dx];
                        if (!(m - 1 > (n ? n - 1 : 0))) k = false;
                    }
                if (k) kv = m;
            }
        }
    }
    keep[pos] = (uint8_t)kv;
    if (kv) atomicAdd(&bins[kv], 1u);
    __syncthreads();
    const u32 c = bins[threadIdx.x];
    if (c) atomicAdd(&hist[l * 256 + threadIdx.x], c);
}

// one wave: lane l turns level l's histogram and quota into cut[l] = (c, r): a kept score v stays when v > c, or v == c and fewer
// than r corners of score c come before it in the level's raster.  Nothing stays at quota 0 (c = 255, r = 0: no v is above 255).
__global__ __launch_bounds__(64) void k_pyr_cut(const u32* __restrict__ hist, vp_pyr_table T, u32* __restrict__ cut)
{
    const int l = threadIdx.x;
    if (l >= T.n_levels) return;
    const u32 q = T.L[l].quota;
    u32 c = 255, r = 0;
    if (q) {
        u32 above = 0;
        c = 0;
        for (int v = 255; v >= 1; v--) {
            const u32 hv = hist[l * 256 + v];
            if (above + hv >= q) { c = (u32)v; r = q - above; break; }
            above += hv;
        }
    }
    cut[2 * l] = c;
    cut[2 * l + 1] = r;
}

// grid as k_pyr_suppress, one wave per FT_CHUNK pixels: gt[chunk] = its kept scores above the level's cutoff, eq[chunk] = those at it
__global__ __launch_bounds__(FT_SEL_BLOCK) void k_pyr_count(const uint8_t* __restrict__ keep, vp_pyr_table T, const u32* __restrict__ cut, u32* __restrict__ gt,
                                                            u32* __restrict__ eq)
{
    const u32 pos = blockIdx.x * FT_SEL_BLOCK + threadIdx.x;
    const int l = pyr_level_of_px(T, blockIdx.x * FT_SEL_BLOCK);
    const u32 c = cut[2 * l], kv = keep[pos];
    const u64 bg = __ballot(kv > c), be = __ballot(kv != 0 && kv == c);
    if ((threadIdx.x & 63) == 0) {
        gt[pos / FT_CHUNK] = (u32)__popcll(bg);
        eq[pos / FT_CHUNK] = (u32)__popcll(be);
    }
}

// a[0 .. chunks) of the one block becomes its exclusive prefix sum in out (which may be a), out[chunks] the total; lane t owns per entries
__device__ __forceinline__ void pyr_block_scan(const u32* a, u32* out, size_t chunks, size_t per, u32* wsum)
{
    const size_t b = (size_t)threadIdx.x * per, e = b + per < chunks ? b + per : chunks;
    u32 s = 0;
    for (size_t i = b; i < e; i++) s += a[i];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 inc = s;
    for (int off = 1; off < 64; off <<= 1) {
        const u32 o = (u32)__shfl_up((int)inc, off);
        if (lane >= off) inc += o;
    }
    __syncthreads();                                       // wsum may still be read from the scan before
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    u32 before = 0;
    for (int q = 0; q < wave; q++) before += wsum[q];
    u32 run = before + inc - s;
    for (size_t i = b; i < e; i++) {
        const u32 c = a[i];
        out[i] = run;
        run += c;
    }
    if (threadIdx.x == FT_SCAN_LANES - 1) out[chunks] = before + inc;
}

// one block of FT_SCAN_LANES lanes.  epre = exclusive prefix of eq over all chunks; the equal-score corners before a chunk inside its
// level are epre[chunk] - epre[first chunk of the level]; the chunk then selects gt + min(eq, r - those) corners; gt becomes the
// exclusive prefix of that, gt[chunks] the number of points.
__global__ __launch_bounds__(FT_SCAN_LANES) void k_pyr_scan(u32* __restrict__ gt, const u32* __restrict__ eq, u32* __restrict__ epre, vp_pyr_table T,
                                                            const u32* __restrict__ cut, size_t chunks, size_t per)
{
    __shared__ u32 wsum[FT_SCAN_LANES / 64];
    pyr_block_scan(eq, epre, chunks, per, wsum);
    __syncthreads();                                       // the block's own writes to epre are visible to all of it from here
    const size_t b = (size_t)threadIdx.x * per, e = b + per < chunks ? b + per : chunks;
    for (size_t i = b; i < e; i++) {
        const int l = pyr_level_of_px(T, (u32)(i * FT_CHUNK));
        const u32 before = epre[i] - epre[T.L[l].off / FT_CHUNK], r = cut[2 * l + 1];
        const u32 room = r > before ? r - before : 0u;
        gt[i] += min(eq[i], room);
    }
    pyr_block_scan(gt, gt, chunks, per, wsum);
}

// grid as k_pyr_suppress: selected corner number offs[chunk] + (selected corners of lower lanes) goes to that slot: (level, x, y) and
// score = kept value - 1.  The quotas sum to the capacity, so every slot exists.
__global__ __launch_bounds__(FT_SEL_BLOCK) void k_pyr_write(const uint8_t* __restrict__ keep, vp_pyr_table T, const u32* __restrict__ cut, const u32* __restrict__ offs,
                                                            const u32* __restrict__ epre, int32_t* __restrict__ lxy, int32_t* __restrict__ val, u32 cap)
{
    const u32 pos = blockIdx.x * FT_SEL_BLOCK + threadIdx.x;
    const int l = pyr_level_of_px(T, blockIdx.x * FT_SEL_BLOCK);
    const vp_pyr_level L = T.L[l];
    const u32 c = cut[2 * l], r = cut[2 * l + 1], kv = keep[pos];
    const int lane = threadIdx.x & 63;
    const u64 below = (1ull << lane) - 1ull;
    const bool iseq = kv != 0 && kv == c;
    const u64 be = __ballot(iseq);
    const u32 chunk = pos / FT_CHUNK;
    bool sel = kv > c;
    if (iseq) sel = epre[chunk] - epre[L.off / FT_CHUNK] + (u32)__popcll(be & below) < r;
    const u64 bs = __ballot(sel);
    if (sel) {
        const u32 slot = offs[chunk] + (u32)__popcll(bs & below);
        if (slot < cap) {
            const u32 i = pos - L.off;
            const int y = (int)(i / (u32)L.w), x = (int)(i - (u32)y * (u32)L.w);
            lxy[3 * (size_t)slot] = l;
            lxy[3 * (size_t)slot + 1] = x;
            lxy[3 * (size_t)slot + 2] = y;
            val[slot] = (int32_t)kv - 1;
        }
    }
}

// grid ceil(cap / FT_DESC_WAVES), one wave per selected point; *count points exist.  The orientation from the point's own level, the
// bits from that level's blur.
__global__ __launch_bounds__(64 * FT_DESC_WAVES) void k_pyr_describe(const uint8_t* __restrict__ img, const uint8_t* __restrict__ blur, vp_pyr_table T,
                                                                     const int32_t* __restrict__ lxy, const u32* __restrict__ count, u32 cap,
                                                                     const int8_t* __restrict__ pattern, ft_trig G, u64* __restrict__ desc, uint8_t* __restrict__ bin)
{
    const int lane = threadIdx.x & 63;
    const u32 p = blockIdx.x * FT_DESC_WAVES + (threadIdx.x >> 6);
    if (p >= cap || p >= *count) return;
    const int l = lxy[3 * (size_t)p], x = lxy[3 * (size_t)p + 1], y = lxy[3 * (size_t)p + 2];
    if (l < 0 || l >= T.n_levels) return;
    const vp_pyr_level L = T.L[l];
    if (x < FT_DESC_BORDER || x > L.w - 1 - FT_DESC_BORDER || y < FT_DESC_BORDER || y > L.h - 1 - FT_DESC_BORDER) return;
    const int kb = describe_pixel(img + L.off, (size_t)L.w, blur + L.off, L.w, x, y, lane, pattern, G, desc + 4 * (size_t)p);
    if (lane == 0) bin[p] = (uint8_t)kb;
}

// ---- Hamming matcher -----------------------------------------------------------------------------------------------------------------
// (d, i) into the best two (d0, i0) <= (d1, i1): a strict "<" on the distance, so among equal distances the one that came first stays
#define HM_INSERT(d, i, d0, i0, d1, i1)                    \
    do {                                                   \
        const int d__ = (d), i__ = (i);                    \
        const bool a__ = d__ < d0, b__ = d__ < d1;         \
        d1 = a__ ? d0 : (b__ ? d__ : d1);                  \
        i1 = a__ ? i0 : (b__ ? i__ : i1);                  \
        d0 = a__ ? d__ : d0;                               \
        i0 = a__ ? i__ : i0;                               \
    } while (0)

__device__ __forceinline__ void hm_store(int32_t* idx, int32_t* dist, size_t q, int k, int d0, int i0, int d1, int i1)
{
    idx[q * k] = i0;
    dist[q * k] = i0 < 0 ? -1 : d0;
    if (k == 2) {
        idx[q * 2 + 1] = i1;
        dist[q * 2 + 1] = i1 < 0 ? -1 : d1;
    }
}

// grid (query_tiles, train_splits), HM_QB lanes.  A lane keeps its query's WP words in registers; the block stages HM_TILE train rows at a
// time in LDS and every lane reads the same row (a broadcast).  The rows of a split are visited in ascending order, so a strict "<"
// keeps the lower index among equal distances.  One split: the results go out; more: each writes (d0, i0, d1, i1) to
// partial[split][query] and k_hamming_merge finishes.
template <int WP>
__global__ __launch_bounds__(HM_QB) void k_hamming(const uint8_t* __restrict__ q, size_t qstride, int nq, const uint8_t* __restrict__ t, size_t tstride, int nt, int words,
                                                   int split_rows, int k, int32_t* __restrict__ idx, int32_t* __restrict__ dist, int4* __restrict__ partial)
{
    __shared__ u64 tile[HM_TILE * WP];
    const int qi = blockIdx.x * HM_QB + threadIdx.x;
    u64 qw[WP];
#pragma unroll
    for (int x = 0; x < WP; x++) qw[x] = (qi < nq && x < words) ? reinterpret_cast<const u64*>(q + (size_t)qi * qstride)[x] : 0ull;
    const int r0 = blockIdx.y * split_rows, r1 = min(r0 + split_rows, nt);
    int d0 = HM_NONE, d1 = HM_NONE, i0 = -1, i1 = -1;
    for (int base = r0; base < r1; base += HM_TILE) {
        const int rows = min(HM_TILE, r1 - base);
        __syncthreads();
        for (int i = threadIdx.x; i < rows * WP; i += HM_QB) {
            const int r = i / WP, x = i % WP;
            tile[i] = x < words ? reinterpret_cast<const u64*>(t + (size_t)(base + r) * tstride)[x] : 0ull;
        }
        __syncthreads();
        for (int r = 0; r < rows; r++) {
            int d = 0;
#pragma unroll
            for (int x = 0; x < WP; x++) d += __popcll(qw[x] ^ tile[r * WP + x]);
            HM_INSERT(d, base + r, d0, i0, d1, i1);
        }
    }
    if (qi >= nq) return;
    if (gridDim.y > 1) partial[(size_t)blockIdx.y * nq + qi] = make_int4(d0, i0, d1, i1);
    else hm_store(idx, dist, (size_t)qi, k, d0, i0, d1, i1);
}

// grid ceil(nq / 256), 256 lanes: the splits in ascending order, so again a strict "<" keeps the lower index
__global__ __launch_bounds__(256) void k_hamming_merge(const int4* __restrict__ partial, int nq, int splits, int k, int32_t* __restrict__ idx, int32_t* __restrict__ dist)
{
    const int qi = blockIdx.x * 256 + threadIdx.x;
    if (qi >= nq) return;
    int d0 = HM_NONE, d1 = HM_NONE, i0 = -1, i1 = -1;
    for (int s = 0; s < splits; s++) {
        const int4 p = partial[(size_t)s * nq + qi];
        if (p.y >= 0) HM_INSERT(p.x, p.y, d0, i0, d1, i1);
        if (p.w >= 0) HM_INSERT(p.z, p.w, d0, i0, d1, i1);
    }
    hm_store(idx, dist, (size_t)qi, k, d0, i0, d1, i1);
}

// grid ceil(nq / 256): a match i -> j stays when j's best query is i
__global__ __launch_bounds__(256) void k_hamming_cross(int32_t* __restrict__ idx, const int32_t* __restrict__ rev, int nq)
{
    const int qi = blockIdx.x * 256 + threadIdx.x;
    if (qi >= nq) return;
    const int j = idx[qi];
    if (j >= 0 && rev[j] != qi) idx[qi] = -1;
}

template <int WP>
void hm_launch(vp_ctx* ctx, const vp_hamming_plan_t& P, const uint8_t* d_q, size_t qstride, int nq, const uint8_t* d_t, size_t tstride, int nt, int k, int32_t* d_idx,
               int32_t* d_dist, int4* d_partial)
{
    hipLaunchKernelGGL(k_hamming<WP>, dim3((unsigned)P.query_tiles, (unsigned)P.train_splits), dim3(HM_QB), 0, ctx->stream, d_q, qstride, nq, d_t, tstride, nt, P.words,
                       P.split_rows, k, d_idx, d_dist, d_partial);
}

}  // namespace

// arguments as vp_fast_refusal admitted them and the plan vp_fast_make_plan made of them; d_ws: P.ws_bytes of workspace, 256-byte
// aligned.  Leaves the count at P.off_cnt + 4 P.chunks and the first min(count, P.out_cap) corners, in raster order, at P.off_xy
// (x, y pairs) and P.off_val (scores).  Four launches, enqueued.
int vpk_fast(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int threshold, int nonmax, const vp_fast_plan& P, uint8_t* d_ws)
{
    const size_t npx = (size_t)w * h;
    uint8_t* d_score = d_ws + P.off_score;
    uint8_t* d_keep = d_ws + P.off_keep;
    u32* d_cnt = reinterpret_cast<u32*>(d_ws + P.off_cnt);
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_fast_score, dim3(P.tiles_x, P.tiles_y), dim3(256), 0, ctx->stream, d_src, stride, w, h, threshold, d_score);
    }
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_fast_count, dim3(P.sel_blocks), dim3(FT_SEL_BLOCK), 0, ctx->stream, d_score, w, npx, nonmax, d_keep, d_cnt);
    }
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_fast_scan, dim3(1), dim3(FT_SCAN_LANES), 0, ctx->stream, d_cnt, P.chunks, P.scan_per_lane);
    }
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_fast_write, dim3(P.sel_blocks), dim3(FT_SEL_BLOCK), 0, ctx->stream, d_keep, w, npx, d_cnt, nonmax,
                           reinterpret_cast<int32_t*>(d_ws + P.off_xy), reinterpret_cast<int32_t*>(d_ws + P.off_val), P.out_cap);
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

// n >= 1 points of an image vp_describe_refusal admitted; d_blur: its packed 7 x 7 Gaussian blur; d_pattern: the FT_PATTERN_BYTES table;
// d_desc 8-byte aligned.  One launch, enqueued.
int vpk_describe(vp_ctx* ctx, const uint8_t* d_src, size_t stride, const uint8_t* d_blur, int w, int h, const float* d_pts, int n, const int8_t* d_pattern,
                 unsigned grid, uint8_t* d_desc, uint8_t* d_bin, uint8_t* d_status)
{
    ft_trig T;
    for (int k = 0; k < FT_BINS; k++) { T.c[k] = vp_ft_cos[k]; T.s[k] = vp_ft_sin[k]; }
    vp_prof_scope ps(ctx, VPK_OTHER);
    hipLaunchKernelGGL(k_describe, dim3(grid), dim3(64 * FT_DESC_WAVES), 0, ctx->stream, d_src, stride, d_blur, w, h, d_pts, n, d_pattern, T,
                       reinterpret_cast<u64*>(d_desc), d_bin, d_status);
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

// nq, nt >= 1 rows as vp_hamming_refusal admitted them and the plan vp_hamming_make_plan made of them; d_partial: P.partial_bytes of
// workspace, 16-byte aligned (unused with one split).  d_idx, d_dist: (nq, k).  One launch, or two with the merge; enqueued.
int vpk_hamming_knn(vp_ctx* ctx, const uint8_t* d_q, size_t qstride, int nq, const uint8_t* d_t, size_t tstride, int nt, const vp_hamming_plan_t& P, int k,
                    int32_t* d_idx, int32_t* d_dist, void* d_partial)
{
    int4* part = reinterpret_cast<int4*>(d_partial);
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        switch (P.words_padded) {
            case 1: hm_launch<1>(ctx, P, d_q, qstride, nq, d_t, tstride, nt, k, d_idx, d_dist, part); break;
            case 2: hm_launch<2>(ctx, P, d_q, qstride, nq, d_t, tstride, nt, k, d_idx, d_dist, part); break;
            case 4: hm_launch<4>(ctx, P, d_q, qstride, nq, d_t, tstride, nt, k, d_idx, d_dist, part); break;
            case 8: hm_launch<8>(ctx, P, d_q, qstride, nq, d_t, tstride, nt, k, d_idx, d_dist, part); break;
            default: hm_launch<16>(ctx, P, d_q, qstride, nq, d_t, tstride, nt, k, d_idx, d_dist, part); break;
        }
    }
    VP_HIP(ctx, hipGetLastError());
    if (P.train_splits > 1) {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_hamming_merge, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ctx->stream, part, nq, P.train_splits, k, d_idx, d_dist);
        VP_HIP(ctx, hipGetLastError());
    }
    return VP_OK;
}

// d_idx: (nq,) best train row of each query; d_rev: best query of each train row; one launch, enqueued
int vpk_hamming_cross(vp_ctx* ctx, int32_t* d_idx, const int32_t* d_rev, int nq)
{
    vp_prof_scope ps(ctx, VPK_OTHER);
    hipLaunchKernelGGL(k_hamming_cross, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ctx->stream, d_idx, d_rev, nq);
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

// Everything after the pyramid and its blurs, for a plan vp_pyr_make_plan made with at least one level and a capacity of at least one
// point; d_ws: P.ws_bytes of workspace, 256-byte aligned, with the levels at P.off_img and their blurs at P.off_blur; d_desc: P.cap
// rows of 32 bytes, 8-byte aligned.  Leaves the number of points at P.off_gt + 4 P.chunks, (level, x, y) at P.off_lxy, the scores at
// P.off_val, the bins at P.off_bin.  One memset and seven launches whatever the number of levels; enqueued.
int vpk_pyr_features(vp_ctx* ctx, const vp_pyr_plan& P, int threshold, const int8_t* d_pattern, uint8_t* d_ws, uint8_t* d_desc)
{
    const vp_pyr_table& T = P.T;
    const uint8_t* d_img = d_ws + P.off_img;
    uint8_t* d_score = d_ws + P.off_score;
    uint8_t* d_keep = d_ws + P.off_keep;
    u32* d_hist = reinterpret_cast<u32*>(d_ws + P.off_hist);
    u32* d_cut = d_hist + FT_PYR_MAX_LEVELS * 256;
    u32* d_gt = reinterpret_cast<u32*>(d_ws + P.off_gt);
    u32* d_eq = reinterpret_cast<u32*>(d_ws + P.off_eq);
    u32* d_epre = reinterpret_cast<u32*>(d_ws + P.off_epre);
    int32_t* d_lxy = reinterpret_cast<int32_t*>(d_ws + P.off_lxy);
    int32_t* d_val = reinterpret_cast<int32_t*>(d_ws + P.off_val);
    ft_trig G;
    for (int k = 0; k < FT_BINS; k++) { G.c[k] = vp_ft_cos[k]; G.s[k] = vp_ft_sin[k]; }
    VP_HIP(ctx, hipMemsetAsync(d_hist, 0, FT_PYR_HIST_BYTES, ctx->stream));
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_pyr_score, dim3(T.total_tiles), dim3(256), 0, ctx->stream, d_img, T, threshold, d_score);
    }
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_pyr_suppress, dim3(P.sel_blocks), dim3(FT_SEL_BLOCK), 0, ctx->stream, d_score, T, d_keep, d_hist);
    }
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_pyr_cut, dim3(1), dim3(64), 0, ctx->stream, d_hist, T, d_cut);
    }
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_pyr_count, dim3(P.sel_blocks), dim3(FT_SEL_BLOCK), 0, ctx->stream, d_keep, T, d_cut, d_gt, d_eq);
    }
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_pyr_scan, dim3(1), dim3(FT_SCAN_LANES), 0, ctx->stream, d_gt, d_eq, d_epre, T, d_cut, P.chunks, P.scan_per_lane);
    }
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_pyr_write, dim3(P.sel_blocks), dim3(FT_SEL_BLOCK), 0, ctx->stream, d_keep, T, d_cut, d_gt, d_epre, d_lxy, d_val, (u32)P.cap);
    }
    {
        vp_prof_scope ps(ctx, VPK_OTHER);
        hipLaunchKernelGGL(k_pyr_describe, dim3(P.desc_grid), dim3(64 * FT_DESC_WAVES), 0, ctx->stream, d_img, d_ws + P.off_blur, T, d_lxy, d_gt + P.chunks, (u32)P.cap,
                           d_pattern, G, reinterpret_cast<u64*>(d_desc), d_ws + P.off_bin);
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
