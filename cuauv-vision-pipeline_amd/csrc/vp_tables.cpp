// Host-side generation of the integer tables OpenCV's 8-bit colour conversions use
// (imgproc/src/color_lab.cpp initLabTabs / RGB2Lab_b ctor, color_hsv.simd.hpp RGB2HSV_b).
// OpenCV evaluates them with softfloat: binary32 for x = i/255 and the cube root result,
// binary64 inside pow() and the cube-root polynomial, round-half-even everywhere.  Ordinary
// IEEE float/double reproduce that as long as nothing is contracted into an FMA, hence
// -ffp-contract=off for this file (see build.py).
#include <cmath>
#include <cstdint>
#include <cstring>
#include "../../include/vp.h"
#include "vp_lab_coeffs.h"

static int round_even(double v) { return (int)std::nearbyint(v); }
static int round_even(float v) { return (int)std::nearbyintf(v); }

// cv::cubeRoot for binary32: cube root of the exponent by integer division, mantissa by a
// quartic rational minimax (evaluated in binary64, rounded once to binary32).
static float cube_root32(float x)
{
    uint32_t bits;
    std::memcpy(&bits, &x, 4);
    if ((bits << 1) == 0) return 0.0f;
    const uint32_t sign = bits & 0x80000000u;
    const uint32_t mag = bits & 0x7fffffffu;
    int e = (int)(mag >> 23) - 127;
    int rem = e % 3;
    if (rem >= 0) rem -= 3;              // rem in {-3,-2,-1}
    const int e3 = (e - rem) / 3;
    uint32_t mbits = (mag & 0x007fffffu) | ((uint32_t)(rem + 127) << 23);
    float mant;
    std::memcpy(&mant, &mbits, 4);       // in [0.125, 1)
    const double t = mant;
    const double p = ((((45.2548339756803022511987494 * t + 192.2798368355061050458134625) * t +
                        119.1654824285581628956914143) * t + 13.43250139086239872172837314) * t +
                      0.1636161226585754240958355063);
    const double q = ((((14.80884093219134573786480845 * t + 151.9714051044435648658557668) * t +
                        168.5254414101568283957668343) * t + 33.9905941350215598754191872) * t + 1.0);
    const float r = (float)(p / q);
    uint32_t rbits;
    std::memcpy(&rbits, &r, 4);
    rbits = (rbits + ((uint32_t)e3 << 23)) | sign;
    float out;
    std::memcpy(&out, &rbits, 4);
    return out;
}

void vp_host_tables(uint16_t* gamma, uint16_t* cbrt_tab, int32_t* sdiv, int32_t* hdiv180, int32_t* labC)
{
    if (gamma)
        for (int i = 0; i < 256; i++) {
            const float xf = (float)i / 255.0f;
            const double x = xf;
            const double lin = x <= 0.04045 ? x / 12.92 : std::pow((x + 0.055) / 1.055, 2.4);
            gamma[i] = (uint16_t)round_even(2040.0f * (float)lin);
        }
    if (cbrt_tab) {
        const float thr = 216.0f / 24389.0f, bias = 16.0f / 116.0f, slope = 841.0f / 108.0f;
        for (int i = 0; i < 3072; i++) {
            const float x = (float)i / 2040.0f;
            const float f = x < thr ? std::fmaf(x, slope, bias) : cube_root32(x);
            cbrt_tab[i] = (uint16_t)round_even(32768.0f * f);
        }
    }
    if (sdiv || hdiv180)
        for (int i = 0; i < 256; i++) {
            if (sdiv) sdiv[i] = i ? round_even((255 << 12) / (double)i) : 0;
            if (hdiv180) hdiv180[i] = i ? round_even((180 << 12) / (6.0 * i)) : 0;
        }
    if (labC) {
        const double m[9] = {0.412453, 0.357580, 0.180423, 0.212671, 0.715160, 0.072169, 0.019334, 0.119193, 0.950227};
        const double white[3] = {0.950456, 1.0, 1.088754};
        for (int k = 0; k < 9; k++) labC[k] = round_even(4096.0 * m[k] / white[k / 3]);
    }
}

// Tables of the 8-bit Lab -> BGR conversion (color_lab.cpp initLabTabs + Lab2RGBinteger ctor).  Same evaluation rules as above:
// LabToYF_b in binary32 statement by statement, the inverse gamma in binary64 (softdouble) rounded once to binary32 before the
// scale by 255, abToXZ_b in C integer arithmetic (division truncates toward zero), the matrix in binary64 at compile time (vp_lab_coeffs.h).
//   yf[2 L], yf[2 L + 1]   = y (Q14, 0..16384) and ify = f(y) (Q14, 2260..16384) of the 8-bit L
//   abxz[i - VP_LAB_MIN_AB] = x or z (Q14) of the Q14 value i of f(x) / f(z), i in [VP_LAB_MIN_AB, VP_LAB_MIN_AB + VP_LAB_AB_TAB)
//   inv_gamma[i]           = cvRound(255 * sRGB(i / 4096)), i < 4096
//   coeffs[3 c + j]        = Q12 coefficient of x, y, z (j) in output channel c, c = 0 blue, 1 green, 2 red; white point folded in
void vp_host_lab_inv_tables(uint16_t* yf, int32_t* abxz, uint16_t* inv_gamma, int32_t* coeffs)
{
    const int BASE = 1 << 14;
    if (yf)
        for (int i = 0; i < 256; i++) {
            int y, ify;
            if (i <= 20) {             // L <= 8: the linear segment, y = L / 903.3 = (i * 100 / 255) * 27 / 24389
                y = round_even((float)(i * BASE * 20 * 9) / (float)(17 * 29 * 29 * 29));
                ify = round_even((float)BASE * (16.0f / 116.0f + (float)(i * 5) / (float)(3 * 17 * 29)));
            } else {                   // fy = (L + 16) / 116, y = fy^3
                const float fy = (float)(i * 100 * BASE) / (float)(255 * 116) + (float)(16 * BASE) / 116.0f;
                ify = round_even(fy);
                y = round_even(fy * fy * fy / (float)(BASE * BASE));
            }
            yf[2 * i] = (uint16_t)y;
            yf[2 * i + 1] = (uint16_t)ify;
        }
    if (abxz)
        for (int i = VP_LAB_MIN_AB; i < VP_LAB_MIN_AB + VP_LAB_AB_TAB; i++) {
            int v;
            if (i <= 3390) v = i * 108 / 841 - BASE * 16 / 116 * 108 / 841;   // (f - 16/116) / 7.787; 6/29 * BASE = 3389.73
            else v = i * i / BASE * i / BASE;                                  // f^3
            abxz[i - VP_LAB_MIN_AB] = v;
        }
    if (inv_gamma) {
        const double thr = 7827.0 / 2500000.0, low = 323.0 / 25.0, power = 12.0 / 5.0, xshift = 11.0 / 200.0;
        for (int i = 0; i < 4096; i++) {
            const double x = (double)((float)i * (1.0f / 4096.0f));
            const float g = (float)(x <= thr ? x * low : std::pow(x, 1.0 / power) * (1.0 + xshift) - xshift);
            inv_gamma[i] = (uint16_t)round_even(255.0f * g);
        }
    }
    if (coeffs)
        for (int k = 0; k < 9; k++) coeffs[k] = VP_LABINV_C[k];
}
