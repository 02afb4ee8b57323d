// Device helpers shared by vp_box.hip, vp_pyr.hip and vp_integral.hip: reads of the border-extended source that never leave the
// image, whatever the alignment of pointer and stride.
#pragma once
#include "vp_internal.h"
#include "vp_box_plan.h"

// 4 bytes at p, any alignment, all four inside the image: one or two aligned dword reads, each of which holds at least one of them
__device__ __forceinline__ u32 bx_ld4(const uint8_t* p)
{
    const uintptr_t a = (uintptr_t)p;
    const u32 sh = (u32)(a & 3u);
    const u32* q = reinterpret_cast<const u32*>(a - sh);
    const u32 lo = q[0];
    if (sh == 0) return lo;
    const u32 hi = q[1];
    return (u32)((((u64)hi << 32) | lo) >> (8 * sh));
}

// bytes g .. g + 3 of an image row of w pixels of CN channels extended by `border` (g >= -2^20 * CN); row: the row's first byte, or
// NULL for a row of the constant border
template <int CN>
__device__ __forceinline__ u32 bx_ext4(const uint8_t* row, int g, int w, int border)
{
    if (!row) return 0;
    if (g >= 0 && g + 4 <= w * CN) return bx_ld4(row + g);
    u32 v = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int gb = g + k;
        const int px = (gb + (1 << 20) * CN) / CN - (1 << 20), c = gb - px * CN;
        const int pm = vp_deriv_border_index(px, w, border);
        if (pm >= 0) v |= (u32)row[(size_t)pm * CN + c] << (8 * k);
    }
    return v;
}
