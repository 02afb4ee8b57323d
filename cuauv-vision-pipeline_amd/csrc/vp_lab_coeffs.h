// The Q12 XYZ -> sRGB matrix of OpenCV's Lab2RGBinteger (color_lab.cpp: cvRound(2^12 * XYZ2sRGB_D65 * D65 white), binary64), computed
// once at compile time from its recipe.  The one definition the host table getter (vp_tables.cpp) and the kernels (vp_lab.h) share.
#pragma once

constexpr double VP_XYZ2SRGB_D65[9] = {3.240479, -1.53715, -0.498535, -0.969256, 1.875991, 0.041556, 0.055648, -0.204043, 1.057311};  // rows R, G, B
constexpr double VP_D65_WHITE[3] = {0.950456, 1.0, 1.088754};

// cvRound of a binary64 value of modest magnitude: round half to even
constexpr int vp_round_even_cx(double v)
{
    long long f = (long long)v;
    if ((double)f > v) f -= 1;                    // floor
    const double d = v - (double)f;               // exact: |v| < 2^31
    if (d > 0.5 || (d == 0.5 && (f & 1))) f += 1;
    return (int)f;
}

// output channel c (0 blue, 1 green, 2 red), input j (0 x, 1 y, 2 z); the products in OpenCV's order, (2^12 * m) * white
constexpr int vp_labinv_coeff(int c, int j) { return vp_round_even_cx(4096.0 * VP_XYZ2SRGB_D65[3 * (2 - c) + j] * VP_D65_WHITE[j]); }

constexpr int VP_LABINV_C[9] = {vp_labinv_coeff(0, 0), vp_labinv_coeff(0, 1), vp_labinv_coeff(0, 2),
                                vp_labinv_coeff(1, 0), vp_labinv_coeff(1, 1), vp_labinv_coeff(1, 2),
                                vp_labinv_coeff(2, 0), vp_labinv_coeff(2, 1), vp_labinv_coeff(2, 2)};
// every |coefficient| below 2^14: the kernels multiply with 24-bit operands
static_assert(VP_LABINV_C[6] < (1 << 14) && VP_LABINV_C[6] > 0, "Q12 coefficient range");
