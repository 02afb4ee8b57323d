// Per-pixel Lab arithmetic shared by vp_color.hip (conversions, thresholds) and vp_whitebal.hip (white balance).
// OpenCV 4.x 8-bit integer paths: RGB2Lab_b (forward) and Lab2RGBinteger (inverse), tables from vp_tables.cpp.
#pragma once
#include "vp_internal.h"
#include "vp_lab_coeffs.h"

#define LAB_LSHIFT (-1336934)  // -((16*255*32768 + 50)/100)

struct LabLds { uint16_t gamma[256]; uint16_t cbrt[2048]; };
// Lab -> BGR: LabToYF_b and the inverse gamma (5 KiB) live in LDS; abToXZ_b (144 KiB) stays in global memory and is read
// through the caches - in LDS it would leave room for one block per CU and cost 144 KiB of table loads per block.
struct LabInvLds { uint16_t yf[512]; uint8_t invg[4096]; };

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
// signed 24-bit multiply, low 32 bits of the product (full rate; v_mul_lo_u32 runs at a quarter of it).  Spelled as the instruction:
// __mul24 becomes it only where the compiler can bound both operands itself.
__device__ __forceinline__ int mul_i24(int a, int b)
{
    int r;
    asm("v_mul_i32_i24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// NEED bit0 = L, bit1 = a, bit2 = b
template <int NEED>
__device__ __forceinline__ void lab_px(const LabLds& t, int b, int g, int r, int& L, int& A, int& Bc)
{
    const int R = t.gamma[r], G = t.gamma[g], B = t.gamma[b];
    const int fY = t.cbrt[(R * 871 + G * 2929 + B * 296 + 2048) >> 12];
    if (NEED & 1) L = clamp255((296 * fY + LAB_LSHIFT + 16384) >> 15);
    if (NEED & 2) {
        const int fX = t.cbrt[(R * 1777 + G * 1541 + B * 778 + 2048) >> 12];
        A = clamp255((500 * (fX - fY) + (128 << 15) + 16384) >> 15);
    }
    if (NEED & 4) {
        const int fZ = t.cbrt[(R * 73 + G * 448 + B * 3575 + 2048) >> 12];
        Bc = clamp255((200 * (fY - fZ) + (128 << 15) + 16384) >> 15);
    }
}

__device__ __forceinline__ void load_lab_lds(LabLds& s, const vp_tables& tab)
{
    for (int i = threadIdx.x; i < 256; i += blockDim.x) s.gamma[i] = tab.gamma[i];
    for (int i = threadIdx.x; i < 2048; i += blockDim.x) s.cbrt[i] = tab.cbrt[i];
}
__device__ __forceinline__ void load_labinv_lds(LabInvLds& s, const vp_tables& tab)
{
    for (int i = threadIdx.x; i < 512; i += blockDim.x) s.yf[i] = tab.yf[i];
    for (int i = threadIdx.x; i < 1024; i += blockDim.x) reinterpret_cast<u32*>(s.invg)[i] = reinterpret_cast<const u32*>(tab.invg)[i];
}

// Lab2RGBinteger::process for one 8-bit (L, a, b): c0, c1, c2 = blue, green, red.
//   y, ify = LabToYF_b[L] (Q14); a / 500 and b / 200 in Q14 by multiply-shift (OpenCV's approximations, 128 * BASE / 500 = 4194,
//   128 * BASE / 200 - 1 = 10484); x, z = abToXZ_b[ify + adiv], abToXZ_b[ify - bdiv]; the Q12 matrix (white point folded in,
//   VP_LABINV_C) with CV_DESCALE by 14, clamped to [0, 4095] and mapped through the inverse gamma.
// Every index is in range for every 8-bit input: ify + adiv in [-1934, 20545], ify - bdiv in [-8145, 26868], table [-8145, 28719).
__device__ __forceinline__ void lab2bgr_px(const LabInvLds& s, const int32_t* __restrict__ abxz, int L, int a, int b, int& c0, int& c1, int& c2)
{
    const int y = s.yf[2 * L], ify = s.yf[2 * L + 1];
    const int adiv = ((a * (5 * 53687) + (1 << 7)) >> 13) - 4194;
    const int bdiv = ((b * 41943 + (1 << 4)) >> 9) - 10484;
    const int x = abxz[ify + adiv - VP_LAB_MIN_AB];
    const int z = abxz[ify - bdiv - VP_LAB_MIN_AB];
    // |coefficient| < 2^14, x in [-1335, 88231], y <= 16384: 24-bit operands, every sum below 2^31
    constexpr int C0 = VP_LABINV_C[0], C1 = VP_LABINV_C[1], C2 = VP_LABINV_C[2], C3 = VP_LABINV_C[3], C4 = VP_LABINV_C[4],
                  C5 = VP_LABINV_C[5], C6 = VP_LABINV_C[6], C7 = VP_LABINV_C[7], C8 = VP_LABINV_C[8];
    const int vb = (mul_i24(C0, x) + mul_i24(C1, y) + mul_i24(C2, z) + (1 << 13)) >> 14;
    const int vg = (mul_i24(C3, x) + mul_i24(C4, y) + mul_i24(C5, z) + (1 << 13)) >> 14;
    const int vr = (mul_i24(C6, x) + mul_i24(C7, y) + mul_i24(C8, z) + (1 << 13)) >> 14;
    c0 = s.invg[min(max(vb, 0), 4095)];
    c1 = s.invg[min(max(vg, 0), 4095)];
    c2 = s.invg[min(max(vr, 0), 4095)];
}
