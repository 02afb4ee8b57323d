// 8-bit HSV -> BGR and HLS -> BGR (OpenCV's float32 forms behind HSV2RGB_b / HLS2RGB_b), shared by the colour balance (vp_balance.hip) and
// the conversions (vp_color.hip).
#pragma once
#include "vp_internal.h"

__device__ __forceinline__ int cb_sat_round(float x)   // cv::saturate_cast<uchar>(float): round half to even, clamp
{
    const int v = (int)rintf(x);
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// OpenCV color_hsv.simd.hpp HSV2RGB_b -> HSV2RGB_f, vector arithmetic form (v - v*s, v - (v*s)*h, (v - v*s) + (v*s)*h), hrange 180.
// Built with -ffp-contract=off: every product and sum rounds separately, as the universal intrinsics do.
__device__ __forceinline__ void cb_hsv2bgr(int H, int S, int V, int& b, int& g, int& r)
{
    float h = (float)H * (6.f / 180.f);
    const float s = (float)S * (1.f / 255.f), v = (float)V * (1.f / 255.f);
    const float pre = truncf(h);
    h = h - pre;
    const float vs = v * s;
    const float vsh = vs * h;
    const float t1 = v - vs, t2 = v - vsh, t3 = (v - vs) + vsh;
    float sec = truncf(pre * (1.0f / 6.0f));
    sec = pre - sec * 6.0f;
    const int sector = (int)sec;
    // (b, g, r) = tab[{1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}][sector], tab = {v, t1, t2, t3}
    float fb, fg, fr;
    switch (sector) {
    case 0: fb = t1; fg = t3; fr = v; break;
    case 1: fb = t1; fg = v; fr = t2; break;
    case 2: fb = t3; fg = v; fr = t1; break;
    case 3: fb = v; fg = t2; fr = t1; break;
    case 4: fb = v; fg = t1; fr = t3; break;
    default: fb = t2; fg = t1; fr = v; break;
    }
    b = cb_sat_round(fb * 255.f);
    g = cb_sat_round(fg * 255.f);
    r = cb_sat_round(fr * 255.f);
}

// OpenCV color_hsv.simd.hpp HLS2RGB_b -> HLS2RGB_f, scalar statement sequence, hrange 180: h = H * (6 / 180) brought into [0, 6) by one
// subtraction of 6 (H <= 255 gives h < 8.5), l = L * (1 / 255), s = S * (1 / 255).  Every operation rounds separately.
__device__ __forceinline__ void hls2bgr_px(int H, int L, int S, int& b, int& g, int& r)
{
    const float l = (float)L * (1.f / 255.f), s = (float)S * (1.f / 255.f);
    float fb = l, fg = l, fr = l;
    if (S != 0) {
        const float p2 = l <= 0.5f ? l * (1.f + s) : (l + s) - l * s;
        const float p1 = 2.f * l - p2;
        float h = (float)H * (6.f / 180.f);
        if (h >= 6.f) h = h - 6.f;
        const float fl = floorf(h);
        const int sector = (int)fl;
        h = h - fl;
        const float d = p2 - p1;
        const float t2 = p1 + d * (1.f - h), t3 = p1 + d * h;
        // (b, g, r) = tab[{1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}][sector], tab = {p2, p1, t2, t3}
        switch (sector) {
        case 0: fb = p1; fg = t3; fr = p2; break;
        case 1: fb = p1; fg = p2; fr = t2; break;
        case 2: fb = t3; fg = p2; fr = p1; break;
        case 3: fb = p2; fg = t2; fr = p1; break;
        case 4: fb = p2; fg = p1; fr = t3; break;
        default: fb = t2; fg = p1; fr = p2; break;
        }
    }
    b = cb_sat_round(fb * 255.f);
    g = cb_sat_round(fg * 255.f);
    r = cb_sat_round(fr * 255.f);
}
