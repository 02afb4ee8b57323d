// Element-wise operators on packed uint8 device images: mask logic (cv2.bitwise_*), saturating arithmetic (cv2.add / subtract /
// absdiff), per-channel tables (cv2.LUT, and image-with-scalar arithmetic), channel split / merge and cv2.countNonZero.
//
// All of it is streaming work: 1 to 3 bytes read per byte written.  One grid-stride kernel per family; lane = 16 bytes = one 16-B
// store and one 16-B load per source.  Planes of one frame sit at byte offsets inside a shared allocation, so the pointers of one
// call need not agree modulo 16:
//   * the flat families (bitwise, arith, LUT, count) split n bytes into a head of up to 15 bytes that brings DST (count: the source) to
//     a 16-B boundary, 16-B groups, and a tail of up to 15 bytes.  Head and tail are done byte-wise by the first lanes of block 0.  A
//     source that is not 16-B aligned at the first group is read with byte loads into the same registers (al_* = 0): the stores stay wide.
//   * split / merge have up to five pointers: the 16-B forms run when all of them are aligned, otherwise every lane moves its 16 pixels
//     byte-wise.  The last npx % 16 pixels go byte-wise to the first lanes of block 0.
// dst may be one of the sources of the flat families (no __restrict__ there): every lane reads its own 16 bytes before it writes them.
#include "vp_internal.h"
#include <string.h>

namespace {

struct q16 { u32 w[4]; };

__device__ __forceinline__ q16 ld16(const uint8_t* p, bool aligned)
{
    q16 r;
    if (aligned) {
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        r.w[0] = v.x; r.w[1] = v.y; r.w[2] = v.z; r.w[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) r.w[j] = (u32)p[4 * j] | ((u32)p[4 * j + 1] << 8) | ((u32)p[4 * j + 2] << 16) | ((u32)p[4 * j + 3] << 24);
    }
    return r;
}
__device__ __forceinline__ void st16(uint8_t* p, const q16& v, bool aligned)
{
    if (aligned) {
        vp_store16(p, v.w[0], v.w[1], v.w[2], v.w[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 16; k++) p[k] = (uint8_t)(v.w[k >> 2] >> (8 * (k & 3)));
    }
}
#define EW_BYTE(q, i) (((q).w[(i) >> 2] >> (8 * ((i) & 3))) & 255u)

// 0x80 in every byte of w that is not zero
__device__ __forceinline__ u32 nz_high(u32 w) { return (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u; }
// 0xff in every byte of w that is not zero
__device__ __forceinline__ u32 nz_ff(u32 w) { return (nz_high(w) >> 7) * 0xffu; }

__device__ __forceinline__ u32 bit_op(int op, u32 x, u32 y)
{
    switch (op) {
        case VP_BITWISE_AND: return x & y;
        case VP_BITWISE_OR: return x | y;
        case VP_BITWISE_XOR: return x ^ y;
        default: return ~x;
    }
}

// four bytes at a time, two 16-bit lanes per half: no carry or borrow ever crosses a lane
__device__ __forceinline__ u32 add_sat4(u32 a, u32 b)
{
    const u32 M = 0x00ff00ffu, H = 0x01000100u;
    u32 e = (a & M) + (b & M), o = ((a >> 8) & M) + ((b >> 8) & M);
    e = (e | ((e & H) - ((e & H) >> 8))) & M;
    o = (o | ((o & H) - ((o & H) >> 8))) & M;
    return e | (o << 8);
}
__device__ __forceinline__ u32 sub_sat4(u32 a, u32 b)
{
    const u32 M = 0x00ff00ffu, H = 0x01000100u;
    u32 e = ((a & M) | H) - (b & M), o = (((a >> 8) & M) | H) - ((b >> 8) & M);     // 0x100 + a - b per lane: bit 8 says a >= b
    e &= (e & H) - ((e & H) >> 8);
    o &= (o & H) - ((o & H) >> 8);
    return e | (o << 8);
}
__device__ __forceinline__ u32 arith_op(int op, u32 x, u32 y)
{
    switch (op) {
        case VP_ARITH_ADD: return add_sat4(x, y);
        case VP_ARITH_SUB: return sub_sat4(x, y);
        default: return sub_sat4(x, y) | sub_sat4(y, x);
    }
}

// ---- bitwise ----------------------------------------------------------------------------------------------------------------------
// MCN: 0 no mask; 1..4 one mask byte per pixel of MCN channels (non-zero = keep, zero = result 0).  b == nullptr: the second operand is
// the byte replicated in sw.  WBITS (MCN <= 1, head == 0, n a multiple of 64): the result is a 0/255 mask and its bit-packed form goes to
// `bits` from the same registers - the four 16-px groups of a word are four neighbouring lanes (k_inrange_u8_flat).
template <int MCN, bool WBITS>
__global__ __launch_bounds__(256) void k_bitwise_u8(int op, const uint8_t* a, const uint8_t* b, u32 sw, const uint8_t* __restrict__ mask, size_t n, size_t head,
                                                    size_t ngroups, int al_a, int al_b, int al_m, uint8_t* dst, u64* __restrict__ bits)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (size_t g = t; g < ngroups; g += (size_t)gridDim.x * 256) {
        const size_t i0 = head + g * 16;
        const q16 qa = ld16(a + i0, al_a);
        q16 qb, out;
        if (b) qb = ld16(b + i0, al_b);
        else qb.w[0] = qb.w[1] = qb.w[2] = qb.w[3] = sw;
#pragma unroll
        for (int j = 0; j < 4; j++) out.w[j] = bit_op(op, qa.w[j], qb.w[j]);
        if constexpr (MCN == 1) {
            const q16 qm = ld16(mask + i0, al_m);
#pragma unroll
            for (int j = 0; j < 4; j++) out.w[j] &= nz_ff(qm.w[j]);
        } else if constexpr (MCN > 1) {
            const size_t p0 = i0 / MCN;
            const int r0 = (int)(i0 - p0 * MCN);
#pragma unroll
            for (int k = 0; k < 16; k++)
                if (mask[p0 + (r0 + k) / MCN] == 0) out.w[k >> 2] &= ~(0xffu << (8 * (k & 3)));
        }
        st16(dst + i0, out, true);
        if constexpr (WBITS) {
            u32 m = 0;
#pragma unroll
            for (int k = 0; k < 16; k++) m |= ((out.w[k >> 2] >> (8 * (k & 3))) & 1u) << k;
            u64 wv = (u64)m << (16 * (threadIdx.x & 3));
            wv |= __shfl_xor(wv, 1);
            wv |= __shfl_xor(wv, 2);
            if ((threadIdx.x & 3) == 0) bits[g >> 2] = wv;
        }
    }
    const size_t tail0 = head + ngroups * 16, edge = head + (n - tail0);     // < 32 bytes
    if (t < edge) {
        const size_t i = t < head ? t : tail0 + (t - head);
        u32 v = bit_op(op, a[i], b ? (u32)b[i] : sw) & 255u;
        if constexpr (MCN > 0)
            if (mask[i / MCN] == 0) v = 0;
        dst[i] = (uint8_t)v;
    }
}

// ---- saturating arithmetic ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_arith_u8(int op, const uint8_t* a, const uint8_t* b, size_t n, size_t head, size_t ngroups, int al_a, int al_b,
                                                  uint8_t* dst)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (size_t g = t; g < ngroups; g += (size_t)gridDim.x * 256) {
        const size_t i0 = head + g * 16;
        const q16 qa = ld16(a + i0, al_a), qb = ld16(b + i0, al_b);
        q16 out;
#pragma unroll
        for (int j = 0; j < 4; j++) out.w[j] = arith_op(op, qa.w[j], qb.w[j]);
        st16(dst + i0, out, true);
    }
    const size_t tail0 = head + ngroups * 16, edge = head + (n - tail0);
    if (t < edge) {
        const size_t i = t < head ? t : tail0 + (t - head);
        dst[i] = (uint8_t)(arith_op(op, a[i], b[i]) & 255u);
    }
}

// ---- per-channel tables -------------------------------------------------------------------------------------------------------------
// dst[i] = lut[i % CN][src[i]]: the CN tables travel as a kernel argument and are looked up in LDS
struct lut_tables { u32 w[256]; };     // 4 tables of 256 bytes
template <int CN>
__global__ __launch_bounds__(256) void k_lut_u8(const uint8_t* src, lut_tables L, size_t n, size_t head, size_t ngroups, int al_s, uint8_t* dst)
{
    __shared__ u32 s_w[256];
    s_w[threadIdx.x] = L.w[threadIdx.x];
    __syncthreads();
    const uint8_t* s = reinterpret_cast<const uint8_t*>(s_w);
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (size_t g = t; g < ngroups; g += (size_t)gridDim.x * 256) {
        const size_t i0 = head + g * 16;
        const int c0 = (int)(i0 % CN);
        const q16 q = ld16(src + i0, al_s);
        q16 out = {{0, 0, 0, 0}};
#pragma unroll
        for (int k = 0; k < 16; k++) out.w[k >> 2] |= (u32)s[((c0 + k) % CN) * 256 + EW_BYTE(q, k)] << (8 * (k & 3));
        st16(dst + i0, out, true);
    }
    const size_t tail0 = head + ngroups * 16, edge = head + (n - tail0);
    if (t < edge) {
        const size_t i = t < head ? t : tail0 + (t - head);
        dst[i] = s[(int)(i % CN) * 256 + src[i]];
    }
}

// ---- split / merge ------------------------------------------------------------------------------------------------------------------
// interleaved CN channels -> planes; a null plane is not written (cv2.extractChannel)
template <int CN>
__global__ __launch_bounds__(256) void k_split_u8(const uint8_t* __restrict__ src, size_t npx, size_t ngroups, int vec, uint8_t* __restrict__ p0,
                                                  uint8_t* __restrict__ p1, uint8_t* __restrict__ p2, uint8_t* __restrict__ p3)
{
    uint8_t* const pl[4] = {p0, p1, p2, p3};
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (size_t g = t; g < ngroups; g += (size_t)gridDim.x * 256) {
        q16 in[CN];
#pragma unroll
        for (int j = 0; j < CN; j++) in[j] = ld16(src + (g * CN + j) * 16, vec);
#pragma unroll
        for (int c = 0; c < CN; c++) {
            if (!pl[c]) continue;
            q16 out = {{0, 0, 0, 0}};
#pragma unroll
            for (int k = 0; k < 16; k++) out.w[k >> 2] |= EW_BYTE(in[(CN * k + c) >> 4], (CN * k + c) & 15) << (8 * (k & 3));
            st16(pl[c] + g * 16, out, vec);
        }
    }
    const size_t done = ngroups * 16;
    if (t < npx - done) {
        const size_t i = done + t;
#pragma unroll
        for (int c = 0; c < CN; c++)
            if (pl[c]) pl[c][i] = src[i * CN + c];
    }
}

template <int CN>
__global__ __launch_bounds__(256) void k_merge_u8(const uint8_t* __restrict__ p0, const uint8_t* __restrict__ p1, const uint8_t* __restrict__ p2,
                                                  const uint8_t* __restrict__ p3, size_t npx, size_t ngroups, int vec, uint8_t* __restrict__ dst)
{
    const uint8_t* const pl[4] = {p0, p1, p2, p3};
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (size_t g = t; g < ngroups; g += (size_t)gridDim.x * 256) {
        q16 in[CN];
#pragma unroll
        for (int c = 0; c < CN; c++) in[c] = ld16(pl[c] + g * 16, vec);
#pragma unroll
        for (int j = 0; j < CN; j++) {
            q16 out = {{0, 0, 0, 0}};
#pragma unroll
            for (int k = 0; k < 16; k++) out.w[k >> 2] |= EW_BYTE(in[(16 * j + k) % CN], (16 * j + k) / CN) << (8 * (k & 3));
            st16(dst + (g * CN + j) * 16, out, vec);
        }
    }
    const size_t done = ngroups * 16;
    if (t < npx - done) {
        const size_t i = done + t;
#pragma unroll
        for (int c = 0; c < CN; c++) dst[i * CN + c] = pl[c][i];
    }
}

// ---- countNonZero -------------------------------------------------------------------------------------------------------------------
// per lane a running count, one wave reduction, one atomic per block into *total (zeroed by the caller on the same stream)
__global__ __launch_bounds__(256) void k_count_nonzero_u8(const uint8_t* __restrict__ src, size_t n, size_t head, size_t ngroups, u64* __restrict__ total)
{
    __shared__ u32 s_part[4];
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    u32 cnt = 0;
    for (size_t g = t; g < ngroups; g += (size_t)gridDim.x * 256) {
        const q16 q = ld16(src + head + g * 16, true);
        cnt += __popc(nz_high(q.w[0])) + __popc(nz_high(q.w[1])) + __popc(nz_high(q.w[2])) + __popc(nz_high(q.w[3]));
    }
    const size_t tail0 = head + ngroups * 16, edge = head + (n - tail0);
    if (t < edge) cnt += src[t < head ? t : tail0 + (t - head)] != 0;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) cnt += __shfl_down(cnt, d);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const u32 sum = s_part[0] + s_part[1] + s_part[2] + s_part[3];
        if (sum) atomicAdd(total, (u64)sum);
    }
}

// ---- convertScaleAbs (alpha 1, beta 0) --------------------------------------------------------------------------------------------
// saturate_cast<uchar>(|v|): integers clamp, floats round half to even first (v_rndne) and NaN gives 0
__device__ __forceinline__ u32 csa_one(uint8_t v) { return v; }
__device__ __forceinline__ u32 csa_one(int16_t v) { return (u32)min(abs((int)v), 255); }
__device__ __forceinline__ u32 csa_one(float v) { const float a = fabsf(v); return a == a ? (a >= 255.0f ? 255u : (u32)rintf(a)) : 0u; }
__device__ __forceinline__ u32 csa_one(double v) { const double a = fabs(v); return a == a ? (a >= 255.0 ? 255u : (u32)rint(a)) : 0u; }

// lane = 16 results = one 16-B store; the 16 source elements are sizeof(S) 16-B loads when al_s (src + head is 16-B aligned), else
// element loads.  Head and tail (see the top of this file) go element by element through the first lanes of block 0.
template <typename S>
__global__ __launch_bounds__(256) void k_convert_scale_abs(const S* __restrict__ src, size_t n, size_t head, size_t ngroups, int al_s, uint8_t* __restrict__ dst)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (size_t g = t; g < ngroups; g += (size_t)gridDim.x * 256) {
        const size_t i0 = head + g * 16;
        union { uint4 q[sizeof(S)]; S v[16]; } in;
        if (al_s) {
#pragma unroll
            for (int j = 0; j < (int)sizeof(S); j++) in.q[j] = reinterpret_cast<const uint4*>(src + i0)[j];
        } else {
#pragma unroll
            for (int k = 0; k < 16; k++) in.v[k] = src[i0 + k];
        }
        u32 out[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 16; k++) out[k >> 2] |= csa_one(in.v[k]) << (8 * (k & 3));
        vp_store16(dst + i0, out[0], out[1], out[2], out[3]);
    }
    if (blockIdx.x == 0) {
        const size_t tail0 = head + ngroups * 16, rest = head + (n - tail0);
        for (size_t i = threadIdx.x; i < rest; i += 256) {
            const size_t at = i < head ? i : tail0 + (i - head);
            dst[at] = (uint8_t)csa_one(src[at]);
        }
    }
}

struct ew_split { size_t head, ngroups; unsigned blocks; };

inline bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// head / 16-B groups of n bytes such that `anchor + head` is 16-B aligned; the grid of k_add_weighted_u8 (16 lanes-bytes x 256 per block),
// capped like the flat colour kernels (the kernels stride over the rest)
ew_split ew_plan(vp_ctx* ctx, const void* anchor, size_t n, bool wide)
{
    ew_split s;
    s.head = wide ? (size_t)((16u - ((uintptr_t)anchor & 15u)) & 15u) : 0;
    if (s.head > n) s.head = n;
    s.ngroups = (n - s.head) / 16;
    size_t blocks = (s.ngroups + 255) / 256;
    const size_t cap = (size_t)(ctx->num_cu > 0 ? ctx->num_cu : 256) * 64;
    if (blocks > cap) blocks = cap;
    s.blocks = (unsigned)(blocks ? blocks : 1);
    return s;
}

}  // namespace

int vpk_bitwise_u8(vp_ctx* ctx, int op, const uint8_t* a, const uint8_t* b, int scalar, const uint8_t* mask, int cn, size_t n, uint8_t* dst, int bits_w, u64* d_bits,
                   int* made_bits)
{
    const ew_split s = ew_plan(ctx, dst, n, true);
    const int mcn = mask ? cn : 0;
    // the bit plane: one byte per pixel, whole words per row, nothing in front of the first group
    const bool wbits = d_bits && bits_w > 0 && bits_w % 64 == 0 && mcn <= 1 && ctx->opt.v[VP_OPT_FLAT_OPS] && s.head == 0 && n % (size_t)bits_w == 0 && al16(d_bits);
    if (made_bits) *made_bits = wbits ? 1 : 0;
    const u32 sw = (u32)(scalar & 255) * 0x01010101u;
    const int al_a = al16(a + s.head) && ctx->opt.v[VP_OPT_FLAT_OPS], al_b = b && al16(b + s.head) && ctx->opt.v[VP_OPT_FLAT_OPS];
    const int al_m = mcn == 1 && al16(mask + s.head) && ctx->opt.v[VP_OPT_FLAT_OPS];
    const dim3 grid(s.blocks), block(256);
#define EW_BITWISE(M, W) hipLaunchKernelGGL((k_bitwise_u8<M, W>), grid, block, 0, ctx->stream, op, a, b, sw, mask, n, s.head, s.ngroups, al_a, al_b, al_m, dst, d_bits)
    switch (mcn) {
        case 0: if (wbits) EW_BITWISE(0, true); else EW_BITWISE(0, false); break;
        case 1: if (wbits) EW_BITWISE(1, true); else EW_BITWISE(1, false); break;
        case 2: EW_BITWISE(2, false); break;
        case 3: EW_BITWISE(3, false); break;
        default: EW_BITWISE(4, false); break;
    }
#undef EW_BITWISE
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

int vpk_arith_u8(vp_ctx* ctx, int op, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* dst)
{
    const ew_split s = ew_plan(ctx, dst, n, true);
    hipLaunchKernelGGL(k_arith_u8, dim3(s.blocks), dim3(256), 0, ctx->stream, op, a, b, n, s.head, s.ngroups, (int)(al16(a + s.head) && ctx->opt.v[VP_OPT_FLAT_OPS]),
                       (int)(al16(b + s.head) && ctx->opt.v[VP_OPT_FLAT_OPS]), dst);
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

int vpk_lut_u8(vp_ctx* ctx, const uint8_t* src, size_t n, int cn, const uint8_t* lut_host, uint8_t* dst)
{
    lut_tables L;
    memset(&L, 0, sizeof(L));
    memcpy(&L, lut_host, (size_t)cn * 256);
    const ew_split s = ew_plan(ctx, dst, n, true);
    const int al_s = al16(src + s.head) && ctx->opt.v[VP_OPT_FLAT_OPS];
    const dim3 grid(s.blocks), block(256);
    switch (cn) {
        case 1: hipLaunchKernelGGL(k_lut_u8<1>, grid, block, 0, ctx->stream, src, L, n, s.head, s.ngroups, al_s, dst); break;
        case 2: hipLaunchKernelGGL(k_lut_u8<2>, grid, block, 0, ctx->stream, src, L, n, s.head, s.ngroups, al_s, dst); break;
        case 3: hipLaunchKernelGGL(k_lut_u8<3>, grid, block, 0, ctx->stream, src, L, n, s.head, s.ngroups, al_s, dst); break;
        default: hipLaunchKernelGGL(k_lut_u8<4>, grid, block, 0, ctx->stream, src, L, n, s.head, s.ngroups, al_s, dst); break;
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

int vpk_split_u8(vp_ctx* ctx, const uint8_t* src, size_t npx, int cn, uint8_t* p0, uint8_t* p1, uint8_t* p2, uint8_t* p3)
{
    const int vec = ctx->opt.v[VP_OPT_FLAT_OPS] && al16(src) && al16(p0) && al16(p1) && al16(p2) && al16(p3);     // (a null plane counts as aligned)
    const ew_split s = ew_plan(ctx, src, npx, false);
    const dim3 grid(s.blocks), block(256);
    switch (cn) {
        case 2: hipLaunchKernelGGL(k_split_u8<2>, grid, block, 0, ctx->stream, src, npx, s.ngroups, vec, p0, p1, p2, p3); break;
        case 3: hipLaunchKernelGGL(k_split_u8<3>, grid, block, 0, ctx->stream, src, npx, s.ngroups, vec, p0, p1, p2, p3); break;
        default: hipLaunchKernelGGL(k_split_u8<4>, grid, block, 0, ctx->stream, src, npx, s.ngroups, vec, p0, p1, p2, p3); break;
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

int vpk_merge_u8(vp_ctx* ctx, const uint8_t* p0, const uint8_t* p1, const uint8_t* p2, const uint8_t* p3, size_t npx, int cn, uint8_t* dst)
{
    const int vec = ctx->opt.v[VP_OPT_FLAT_OPS] && al16(dst) && al16(p0) && al16(p1) && al16(p2) && al16(p3);
    const ew_split s = ew_plan(ctx, dst, npx, false);
    const dim3 grid(s.blocks), block(256);
    switch (cn) {
        case 2: hipLaunchKernelGGL(k_merge_u8<2>, grid, block, 0, ctx->stream, p0, p1, p2, p3, npx, s.ngroups, vec, dst); break;
        case 3: hipLaunchKernelGGL(k_merge_u8<3>, grid, block, 0, ctx->stream, p0, p1, p2, p3, npx, s.ngroups, vec, dst); break;
        default: hipLaunchKernelGGL(k_merge_u8<4>, grid, block, 0, ctx->stream, p0, p1, p2, p3, npx, s.ngroups, vec, dst); break;
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

int vpk_count_nonzero_u8(vp_ctx* ctx, const uint8_t* src, size_t n, u64* d_total)
{
    VP_HIP(ctx, hipMemsetAsync(d_total, 0, sizeof(u64), ctx->stream));
    const ew_split s = ew_plan(ctx, src, n, true);
    hipLaunchKernelGGL(k_count_nonzero_u8, dim3(s.blocks), dim3(256), 0, ctx->stream, src, n, s.head, s.ngroups, d_total);
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}

template <typename S>
static void csa_launch(vp_ctx* ctx, const void* d_src, size_t n, uint8_t* d_dst)
{
    const ew_split s = ew_plan(ctx, d_dst, n, true);
    const S* src = static_cast<const S*>(d_src);
    hipLaunchKernelGGL(k_convert_scale_abs<S>, dim3(s.blocks), dim3(256), 0, ctx->stream, src, n, s.head, s.ngroups, (int)al16(src + s.head), d_dst);
}

int vpk_convert_scale_abs(vp_ctx* ctx, const void* d_src, int depth, size_t n, uint8_t* d_dst)
{
    switch (depth) {
        case VP_DEPTH_8U: csa_launch<uint8_t>(ctx, d_src, n, d_dst); break;
        case VP_DEPTH_16S: csa_launch<int16_t>(ctx, d_src, n, d_dst); break;
        case VP_DEPTH_32F: csa_launch<float>(ctx, d_src, n, d_dst); break;
        default: csa_launch<double>(ctx, d_src, n, d_dst); break;
    }
    VP_HIP(ctx, hipGetLastError());
    return VP_OK;
}
