// cv2.medianBlur on uint8 images: dst[y][x][c] = the median of the ksize x ksize window of channel c centred on (x, y), coordinates
// outside the image clamped to the nearest edge pixel (BORDER_REPLICATE), ksize odd, 1..255.  An order statistic of bytes: nothing is
// rounded, so every kernel here equals OpenCV's three code paths by construction (tests/median_restate.py is the statement).
//
// All kernels see the image as rows of w * cn bytes whose horizontal neighbour is cn bytes away; channels never mix.  The source has
// a row stride, the destination is packed.  Three kernels, chosen by vp_median_make_plan (vp_median_plan.h):
//   k_median_net<K>   K = 3, 5: an LDS tile with its halo, borders already clamped; each thread selects four neighbouring result bytes
//                     with a fixed min/max exchange network and stores them as one dword.
//   k_median_hist     K = 7..255: one lane per result byte column of a strip slides a 256-bin window histogram down the rows
//                     (2 K updates per result, not K * K), 16-bit bins laid out [bin][lane] in LDS beside a 16-bin coarse histogram;
//                     the median is a coarse scan and a fine scan.
//   k_median_mask     K = 3..63 on a single-channel 0/255 mask: the median is a majority vote.  The tile is kept as bits (the source's
//                     bit plane, or a wave ballot over its bytes), a window row is a shift and a popcount of a 64-bit word, the
//                     K row counts are summed down the column; the result's bit plane comes out of the same ballots.
#include "vp_internal.h"
#include "vp_median_plan.h"

namespace {

__device__ __forceinline__ int md_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// ---- windows 3 and 5: exchange networks ---------------------------------------------------------------------------------------------
#define MD_MAXR (MD_NET_MAXK / 2)
#define MD_PAD 8                                   // staged bytes in front of the tile's first result byte: >= MD_MAXR * 4 channels, whole dwords
#define MD_SW (MD_TB + 2 * MD_PAD + 4)             // staged bytes per row: tile, halo, and up to 3 bytes that bring the row's dwords to aligned addresses
#define MD_SH (MD_TH + 2 * MD_MAXR)                // staged rows
static_assert(MD_PAD >= MD_MAXR * 4 && MD_PAD % 4 == 0 && MD_SW % 4 == 0, "k_median_net: the halo of four channels in whole dwords");
static_assert(MD_TB == 256 && MD_TH % 4 == 0, "k_median_net: one wave per result row, 4 result bytes per lane");
static_assert(MD_SH * MD_SW <= 64 * 1024, "k_median_net: static LDS above 64 KiB");

// a <- min, b <- max
#define MD_CX(a, b) { const u32 lo__ = min(p[a], p[b]); p[b] = max(p[a], p[b]); p[a] = lo__; }

// median of 9: 19 exchanges (J. L. Smith's network, as in Paeth, "Median finding on a 3x3 grid", Graphics Gems)
__device__ __forceinline__ u32 md_select9(u32* p)
{
    MD_CX(1, 2) MD_CX(4, 5) MD_CX(7, 8) MD_CX(0, 1) MD_CX(3, 4) MD_CX(6, 7) MD_CX(1, 2) MD_CX(4, 5) MD_CX(7, 8) MD_CX(0, 3)
    MD_CX(5, 8) MD_CX(4, 7) MD_CX(3, 6) MD_CX(1, 4) MD_CX(2, 5) MD_CX(4, 7) MD_CX(4, 2) MD_CX(6, 4) MD_CX(4, 2)
    return p[4];
}

// median of 25: 99 exchanges (N. Devillard, "Fast median search: an ANSI C implementation", 1998); tests/test_median_network.py
// checks both lists over every 0/1 input, which settles them for every input
__device__ __forceinline__ u32 md_select25(u32* p)
{
    MD_CX(0, 1) MD_CX(3, 4) MD_CX(2, 4) MD_CX(2, 3) MD_CX(6, 7) MD_CX(5, 7) MD_CX(5, 6) MD_CX(9, 10) MD_CX(8, 10) MD_CX(8, 9)
    MD_CX(12, 13) MD_CX(11, 13) MD_CX(11, 12) MD_CX(15, 16) MD_CX(14, 16) MD_CX(14, 15) MD_CX(18, 19) MD_CX(17, 19) MD_CX(17, 18) MD_CX(21, 22)
    MD_CX(20, 22) MD_CX(20, 21) MD_CX(23, 24) MD_CX(2, 5) MD_CX(3, 6) MD_CX(0, 6) MD_CX(0, 3) MD_CX(4, 7) MD_CX(1, 7) MD_CX(1, 4)
    MD_CX(11, 14) MD_CX(8, 14) MD_CX(8, 11) MD_CX(12, 15) MD_CX(9, 15) MD_CX(9, 12) MD_CX(13, 16) MD_CX(10, 16) MD_CX(10, 13) MD_CX(20, 23)
    MD_CX(17, 23) MD_CX(17, 20) MD_CX(21, 24) MD_CX(18, 24) MD_CX(18, 21) MD_CX(19, 22) MD_CX(8, 17) MD_CX(9, 18) MD_CX(0, 18) MD_CX(0, 9)
    MD_CX(10, 19) MD_CX(1, 19) MD_CX(1, 10) MD_CX(11, 20) MD_CX(2, 20) MD_CX(2, 11) MD_CX(12, 21) MD_CX(3, 21) MD_CX(3, 12) MD_CX(13, 22)
    MD_CX(4, 22) MD_CX(4, 13) MD_CX(14, 23) MD_CX(5, 23) MD_CX(5, 14) MD_CX(15, 24) MD_CX(6, 24) MD_CX(6, 15) MD_CX(7, 16) MD_CX(7, 19)
    MD_CX(13, 21) MD_CX(15, 23) MD_CX(7, 13) MD_CX(7, 15) MD_CX(1, 9) MD_CX(3, 11) MD_CX(5, 17) MD_CX(11, 17) MD_CX(9, 17) MD_CX(4, 10)
    MD_CX(6, 12) MD_CX(7, 14) MD_CX(4, 6) MD_CX(4, 7) MD_CX(12, 14) MD_CX(10, 14) MD_CX(6, 7) MD_CX(10, 12) MD_CX(6, 10) MD_CX(6, 17)
    MD_CX(12, 17) MD_CX(7, 17) MD_CX(7, 10) MD_CX(12, 18) MD_CX(7, 12) MD_CX(10, 18) MD_CX(12, 20) MD_CX(10, 20) MD_CX(10, 12)
    return p[12];
}

// grid (ceil(w * cn / MD_TB), ceil(h / MD_TH)), 256 threads
template <int K>
__global__ __launch_bounds__(256) void k_median_net(const uint8_t* __restrict__ src, size_t sstride, int w, int h, int cn, uint8_t* __restrict__ dst)
{
    constexpr int R = K / 2;
    __shared__ u32 st32[MD_SH * (MD_SW / 4)];
    const uint8_t* st = reinterpret_cast<const uint8_t*>(st32);
    const int rb = w * cn, t = threadIdx.x;
    const int b0 = blockIdx.x * MD_TB, y0 = blockIdx.y * MD_TH;
    const int nb = min(MD_TB, rb - b0), nrows = min(MD_TH, h - y0);
    const int sh = nrows + 2 * R;                            // staged rows <= MD_SH
    // Staged byte s of a row is row byte b0 - MD_PAD - sft + s, sft = 0..3 chosen per row so that every staged dword sits at a 4-byte
    // aligned address, whatever the source pointer and stride are (a column window of a wider buffer): interior dwords are single loads.
    const int ndw = (nb + 2 * MD_PAD + 3 + 3) / 4;           // staged dwords per row <= MD_SW / 4
    const uintptr_t base = (uintptr_t)src + (uintptr_t)(intptr_t)(b0 - MD_PAD);
    for (int i = t; i < sh * ndw; i += 256) {
        const int j = i / ndw, d = i - j * ndw;
        const size_t roff = (size_t)md_clamp(y0 - R + j, h - 1) * sstride;
        const uint8_t* row = src + roff;
        const int g = b0 - MD_PAD - (int)((base + roff) & 3u) + 4 * d;
        u32 v = 0;
        if (g >= 0 && g + 4 <= rb) {
            v = *reinterpret_cast<const u32*>(row + g);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {                    // a byte left or right of the row is its channel of the edge pixel
                const int gb = g + k;
                const int px = (gb + 12 * cn) / cn - 12, c = gb - px * cn;      // (gb >= -MD_PAD - 3)
                v |= (u32)row[(size_t)md_clamp(px, w - 1) * cn + c] << (8 * k);
            }
        }
        st32[j * (MD_SW / 4) + d] = v;
    }
    __syncthreads();
    const int q = t & 63, o = 4 * q;                         // a wave = one result row: lane q has its bytes o .. o + 3
    if (o >= nb) return;
    const bool wide = o + 4 <= nb && (((uintptr_t)dst | (uintptr_t)rb) & 3u) == 0;
    for (int r = t >> 6; r < nrows; r += 4) {
        const uint8_t* tap[K];                               // per window row: the tap left of result byte o at dx = 0
#pragma unroll
        for (int dy = 0; dy < K; dy++)
            tap[dy] = st + (r + dy) * MD_SW + MD_PAD + (int)((base + (size_t)md_clamp(y0 - R + r + dy, h - 1) * sstride) & 3u) + o - R * cn;
        u32 out = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (o + i < nb) {
                u32 p[K * K];
#pragma unroll
                for (int dy = 0; dy < K; dy++)
#pragma unroll
                    for (int dx = 0; dx < K; dx++) p[dy * K + dx] = tap[dy][i + dx * cn];
                out |= (K == 3 ? md_select9(p) : md_select25(p)) << (8 * i);
            }
        }
        uint8_t* d = dst + (size_t)(y0 + r) * rb + b0 + o;
        if (wide) {
            *reinterpret_cast<u32*>(d) = out;
        } else {
            for (int i = 0; i < 4 && o + i < nb; i++) d[i] = (uint8_t)(out >> (8 * i));
        }
    }
}

// ---- windows 7 .. 255: sliding histograms -------------------------------------------------------------------------------------------
// Two 16-bit bins share a dword: lane l counts in half (l & 1) of word [bin][l >> 1], which is the [bin][lane] layout of 16-bit bins.
// A count never exceeds K * (K + 1) <= 65,280 (the entering row is added before the leaving one is removed), so no half carries into
// its neighbour, and removing from a half that holds the byte never borrows.  The updates are LDS atomics without a return value:
// two lanes may hit one dword in one instruction, and nothing waits for them.
#define MH_WORDS (MH_LANES / 2)
static_assert((256 + 16) * MH_WORDS * 4 <= 64 * 1024, "k_median_hist: static LDS above 64 KiB");
static_assert(255 * 256 < 65536, "k_median_hist: 16-bit bins hold the window plus one entering row");

// grid (ceil(w * cn / MH_LANES), ceil(h / strip_h)), MH_LANES threads
__global__ __launch_bounds__(MH_LANES) void k_median_hist(const uint8_t* __restrict__ src, size_t sstride, int w, int h, int cn, int K, int strip_h,
                                                          uint8_t* __restrict__ dst)
{
    __shared__ u32 fine[256 * MH_WORDS];
    __shared__ u32 coarse[16 * MH_WORDS];
    const int lane = threadIdx.x, rb = w * cn, R = K / 2;
    const int b = blockIdx.x * MH_LANES + lane;
    const bool active = b < rb;
    const int bc = active ? b : rb - 1;                      // lanes past the row count the last column and store nothing
    const int px = bc / cn, c = bc - px * cn;
    const int y0 = blockIdx.y * strip_h, y1 = min(h, y0 + strip_h);
    for (int i = lane; i < 256 * MH_WORDS; i += MH_LANES) fine[i] = 0;
    for (int i = lane; i < 16 * MH_WORDS; i += MH_LANES) coarse[i] = 0;
    __syncthreads();
    const int li = lane >> 1, shift = 16 * (lane & 1);
    const u32 one = 1u << shift;
    const u32 rank = (u32)(K * K) / 2;                       // the median is the value with more than `rank` window bytes at or below it

    auto add_row = [&](int y) {
        const uint8_t* row = src + (size_t)md_clamp(y, h - 1) * sstride + c;
#pragma unroll 4
        for (int dx = -R; dx <= R; dx++) {
            const u32 v = row[(size_t)md_clamp(px + dx, w - 1) * cn];
            atomicAdd(&fine[v * MH_WORDS + li], one);
            atomicAdd(&coarse[(v >> 4) * MH_WORDS + li], one);
        }
    };
    auto remove_row = [&](int y) {
        const uint8_t* row = src + (size_t)md_clamp(y, h - 1) * sstride + c;
#pragma unroll 4
        for (int dx = -R; dx <= R; dx++) {
            const u32 v = row[(size_t)md_clamp(px + dx, w - 1) * cn];
            atomicSub(&fine[v * MH_WORDS + li], one);
            atomicSub(&coarse[(v >> 4) * MH_WORDS + li], one);
        }
    };

    for (int y = y0 - R; y <= y0 + R; y++) add_row(y);
    for (int y = y0; y < y1; y++) {
        __syncthreads();
        u32 sum = 0;
        int cb = 0;
        for (; cb < 15; cb++) {
            const u32 n = (coarse[cb * MH_WORDS + li] >> shift) & 0xffffu;
            if (sum + n > rank) break;
            sum += n;
        }
        int v = cb * 16;
        for (const int last = v + 15; v < last; v++) {
            sum += (fine[v * MH_WORDS + li] >> shift) & 0xffffu;
            if (sum > rank) break;
        }
        if (active) dst[(size_t)y * rb + b] = (uint8_t)v;
        __syncthreads();
        if (y + 1 < y1) {
            add_row(y + 1 + R);
            remove_row(y - R);
        }
    }
}

// ---- single-channel 0/255 masks, windows 3 .. 63: majority vote on bits ---------------------------------------------------------------
#define MM_MAXR (MM_MAXK / 2)
#define MM_WORDS (MM_TW / 64 + 2)                  // staged words per row: the tile's and one halo word on either side (MM_MAXR < 64)
#define MM_SH (MM_TH + 2 * MM_MAXR)                // staged rows
static_assert(MM_TW == 256 && MM_MAXK <= 63, "k_median_mask: one thread per tile column, a window row inside one 64-bit word");
static_assert(MM_SH * MM_WORDS * 8 <= 64 * 1024, "k_median_mask: static LDS above 64 KiB");

// word wi of a row of a bit plane of w pixels, replicated past both ends (and past pixel w - 1 inside the last word)
__device__ __forceinline__ u64 mm_plane_word(const u64* __restrict__ rowbits, int wi, int w)
{
    const int last = (w - 1) >> 6, lastbit = (w - 1) & 63;
    if (wi < 0) return (rowbits[0] & 1ull) ? ~0ull : 0ull;
    if (wi > last) return ((rowbits[last] >> lastbit) & 1ull) ? ~0ull : 0ull;
    u64 v = rowbits[wi];
    if (wi == last && lastbit != 63) {
        const u64 m = (2ull << lastbit) - 1ull;
        v = ((v >> lastbit) & 1ull) ? (v | ~m) : (v & m);
    }
    return v;
}

// grid (ceil(w / MM_TW), ceil(h / MM_TH)), 256 threads.  bits_in (FROM_BITS): vp_ww(w) words per row, bit x & 63 of word x >> 6 is
// pixel x (what vp_bitwise_u8_dev and vp_inrange_u8_bits_dev write).  bits_out (nullable, w % 64 == 0 only): the result in that layout.
template <bool FROM_BITS>
__global__ __launch_bounds__(256) void k_median_mask(const uint8_t* __restrict__ src, size_t sstride, const u64* __restrict__ bits_in, int w, int h, int K,
                                                     uint8_t* __restrict__ dst, u64* __restrict__ bits_out)
{
    __shared__ u64 sb[MM_SH * MM_WORDS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, R = K / 2;
    const int x0 = blockIdx.x * MM_TW, y0 = blockIdx.y * MM_TH;
    const int nrows = min(MM_TH, h - y0), sh = nrows + 2 * R;        // staged rows <= MM_SH; staged word q holds pixels x0 - 64 + 64 q ..
    if constexpr (FROM_BITS) {
        const int ww = (w + 63) >> 6;
        for (int i = t; i < sh * MM_WORDS; i += 256) {
            const int j = i / MM_WORDS, q = i - j * MM_WORDS;
            sb[i] = mm_plane_word(bits_in + (size_t)md_clamp(y0 - R + j, h - 1) * ww, (x0 >> 6) - 1 + q, w);
        }
    } else {
        for (int i = wave; i < sh * MM_WORDS; i += 4) {              // one word per wave and turn: 64 bytes, one ballot
            const int j = i / MM_WORDS, q = i - j * MM_WORDS;
            const bool need = (q >= 1 && q <= MM_WORDS - 2) || (q == 0 && lane >= 64 - R) || (q == MM_WORDS - 1 && lane < R);
            const int x = md_clamp(x0 - 64 + 64 * q + lane, w - 1);
            const uint8_t v = need ? src[(size_t)md_clamp(y0 - R + j, h - 1) * sstride + x] : (uint8_t)0;
            const u64 word = __ballot(v != 0);
            if (lane == 0) sb[i] = word;
        }
    }
    __syncthreads();
    const int x = x0 + t;
    const int p = 64 + t - R, wq = p >> 6, s = p & 63;               // the window row of column t starts at staged bit p
    const u64 km = (1ull << K) - 1ull;
    auto row_count = [&](int j) {
        const u64 lo = sb[j * MM_WORDS + wq], hi = sb[j * MM_WORDS + wq + 1];
        const u64 win = s ? ((lo >> s) | (hi << (64 - s))) : lo;
        return (int)__popcll(win & km);
    };
    int cnt = 0;
    for (int j = 0; j < K - 1; j++) cnt += row_count(j);
    const int half = K * K / 2;
    const bool wbits = bits_out != nullptr && x0 + 64 * wave < w;    // (whole words per row: a wave is inside the image or outside it)
    for (int r = 0; r < nrows; r++) {
        cnt += row_count(r + K - 1);
        const bool on = cnt > half;
        if (x < w) dst[(size_t)(y0 + r) * w + x] = on ? (uint8_t)255 : (uint8_t)0;
        const u64 word = __ballot(on);
        if (wbits && lane == 0) bits_out[(size_t)(y0 + r) * (w >> 6) + (x0 >> 6) + wave] = word;
        cnt -= row_count(r);
    }
}

}  // namespace

// sstride: bytes between source rows; d_src_bits / d_dst_bits (nullable): bit planes of a single-channel mask (binary_hint); *made_bits
// (nullable) is written only when the launch went out
int vpk_median_blur(vp_ctx* ctx, const uint8_t* d_src, size_t sstride, int w, int h, int cn, int ksize, int binary_hint, const u64* d_src_bits, uint8_t* d_dst,
                    u64* d_dst_bits, int* made_bits)
{
    const vp_median_plan P = vp_median_make_plan(w, h, cn, ksize, binary_hint, d_src_bits != nullptr, d_dst_bits != nullptr, ctx->opt.v[VP_OPT_MEDIAN_MASK]);
    const size_t rowbytes = (size_t)w * cn;
    vp_prof_scope ps(ctx, VPK_OTHER);
    const dim3 grid(P.gx, P.gy), block(P.block);
    switch (P.kernel) {
        case VP_MEDIAN_COPY:
            VP_HIP(ctx, hipMemcpy2DAsync(d_dst, rowbytes, d_src, sstride, rowbytes, h, hipMemcpyDeviceToDevice, ctx->stream));
            break;
        case VP_MEDIAN_NETWORK:
            if (ksize == 3) hipLaunchKernelGGL(k_median_net<3>, grid, block, 0, ctx->stream, d_src, sstride, w, h, cn, d_dst);
            else hipLaunchKernelGGL(k_median_net<5>, grid, block, 0, ctx->stream, d_src, sstride, w, h, cn, d_dst);
            break;
        case VP_MEDIAN_HIST:
            hipLaunchKernelGGL(k_median_hist, grid, block, 0, ctx->stream, d_src, sstride, w, h, cn, ksize, P.strip_h, d_dst);
            break;
        default: {
            u64* out_bits = P.write_bits ? d_dst_bits : nullptr;
            if (P.from_bits) hipLaunchKernelGGL(k_median_mask<true>, grid, block, 0, ctx->stream, d_src, sstride, d_src_bits, w, h, ksize, d_dst, out_bits);
            else hipLaunchKernelGGL(k_median_mask<false>, grid, block, 0, ctx->stream, d_src, sstride, d_src_bits, w, h, ksize, d_dst, out_bits);
            break;
        }
    }
    VP_HIP(ctx, hipGetLastError());
    if (made_bits) *made_bits = (P.kernel == VP_MEDIAN_MASK && P.write_bits) ? 1 : 0;
    return VP_OK;
}
