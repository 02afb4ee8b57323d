"""Restatement, in numpy integers and binary32 / binary64 scalars, of OpenCV 4.x's 8-bit COLOR_Lab2BGR (Lab2RGBinteger,
imgproc/src/color_lab.cpp, tables from initLabTabs) and of the reference's white_balance_bgr / white_balance_bgr_blur
(utils/color.py:370-392).  Independent of libvp's C++: every table is rebuilt here from OpenCV's formulas.

Constants and where their values come from (color_lab.cpp):
  BASE = 1 << 14          Lab2RGBinteger::base_shift = 14: y, f(y), x, z are Q14
  LAB_SHIFT = 12          lab_shift = xyz_shift = 12: the matrix coefficients are Q12
  INV_GAMMA_SHIFT = 12    inv_gamma_shift; INV_GAMMA_TAB_SIZE = 1 << 12 entries of sRGBInvGammaTab_b
  DESCALE = 14            Lab2RGBinteger::shift = lab_shift + (base_shift - inv_gamma_shift): Q12 * Q14 -> Q12 index
  MIN_AB = -8145          minABvalue: the smallest ify - bdiv over all 8-bit inputs (2260 - 10405)
  AB_TAB = BASE * 9 // 4  size of abToXZ_b (36864): covers ify + adiv and ify - bdiv up to 26868
  L_LINEAR_MAX = 20       8-bit L <= 20 (L* <= 8 = 20.4 / 2.55) takes the linear segment y = L* / 903.3
  AB_CUBE_MIN = 3391      abToXZ_b: f <= 3390 (6/29 * BASE = 3389.73) inverts the linear segment, above it f^3
  ADIV: a * BASE / 500 as ((5 a 53687 + 2^7) >> 13) - 128 BASE / 500 (= 4194, C integer division)
  BDIV: b * BASE / 200 as ((b 41943 + 2^4) >> 9) - 128 BASE / 200 + 1 (= -10484)
  XYZ2sRGB_D65 = (3.240479, -1.53715, -0.498535; -0.969256, 1.875991, 0.041556; 0.055648, -0.204043, 1.057311), D65 white
  (0.950456, 1, 1.088754); coefficient = cvRound((2^12 * m) * white[column]) in binary64, rows of the output B, G, R.
  sRGB inverse gamma (applyInvGamma): x <= 7827 / 2500000 -> 12.92 x, else 1.055 x^(1/2.4) - 0.055 (binary64, then binary32).
cvRound is round-half-even; numpy's float32 scalar arithmetic is IEEE binary32 with round-to-nearest, as OpenCV's softfloat.
"""
from fractions import Fraction

import numpy as np

BASE = 1 << 14
LAB_SHIFT = 12
INV_GAMMA_SHIFT = 12
INV_GAMMA_TAB_SIZE = 1 << INV_GAMMA_SHIFT
DESCALE = LAB_SHIFT + (14 - INV_GAMMA_SHIFT)
MIN_AB = -8145
AB_TAB = BASE * 9 // 4
L_LINEAR_MAX = 20
AB_CUBE_MIN = 3391
ADIV_BIAS = 128 * BASE // 500
BDIV_BIAS = 128 * BASE // 200 - 1
XYZ2SRGB = ((3.240479, -1.53715, -0.498535), (-0.969256, 1.875991, 0.041556), (0.055648, -0.204043, 1.057311))
WHITE = (0.950456, 1.0, 1.088754)
GAMMA_INV_THRESHOLD = 7827 / 2500000
GAMMA_LOW_SCALE = 323 / 25
GAMMA_POWER = 12 / 5
GAMMA_XSHIFT = 11 / 200

f32 = np.float32


def _rint(v):
    return int(np.rint(v))


def _cdiv(a, b):
    """C integer division (truncation toward zero)."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def lab_to_yf():
    """LabToYF_b as (256, 2): (y, ify) per 8-bit L, binary32 statement by statement."""
    out = np.zeros((256, 2), np.int64)
    for i in range(256):
        if i <= L_LINEAR_MAX:
            y = _rint(f32(i * BASE * 20 * 9) / f32(17 * 29 * 29 * 29))
            ify = _rint(f32(BASE) * (f32(16) / f32(116) + f32(i * 5) / f32(3 * 17 * 29)))
        else:
            fy = f32(i * 100 * BASE) / f32(255 * 116) + f32(16 * BASE) / f32(116)
            ify = _rint(fy)
            y = _rint(fy * fy * fy / f32(BASE * BASE))
        out[i] = (y, ify)
    return out


def ab_to_xz():
    """abToXZ_b: entry i - MIN_AB is x (or z) in Q14 for the Q14 value i of f(x) (or f(z))."""
    i = np.arange(MIN_AB, MIN_AB + AB_TAB, dtype=np.int64)
    lin = np.array([_cdiv(int(v) * 108, 841) for v in i[i < AB_CUBE_MIN]], np.int64) - _cdiv(_cdiv(BASE * 16, 116) * 108, 841)
    cube = (i[i >= AB_CUBE_MIN] * i[i >= AB_CUBE_MIN] // BASE) * i[i >= AB_CUBE_MIN] // BASE   # non-negative: // = C division
    return np.concatenate([lin, cube])


def inv_gamma_arg(i):
    """The binary32 value cvRound sees for sRGBInvGammaTab_b[i]: 255 * float32(applyInvGamma(i / 4096))."""
    x = float(f32(i) * f32(1.0 / INV_GAMMA_TAB_SIZE))
    g = x * GAMMA_LOW_SCALE if x <= GAMMA_INV_THRESHOLD else x ** (1.0 / GAMMA_POWER) * (1.0 + GAMMA_XSHIFT) - GAMMA_XSHIFT
    return f32(255) * f32(g)


def inv_gamma():
    return np.array([_rint(inv_gamma_arg(i)) for i in range(INV_GAMMA_TAB_SIZE)], np.int64)


def coeff_args():
    """(3, 3) binary64 arguments of cvRound for the Q12 matrix, rows B, G, R of the output, columns x, y, z."""
    rows = (XYZ2SRGB[2], XYZ2SRGB[1], XYZ2SRGB[0])
    return np.array([[(float(1 << LAB_SHIFT) * rows[c][j]) * WHITE[j] for j in range(3)] for c in range(3)])


def coeffs():
    return np.rint(coeff_args()).astype(np.int64)


class Tables:
    def __init__(self):
        self.yf = lab_to_yf()
        self.abxz = ab_to_xz()
        self.invg = inv_gamma()
        self.C = coeffs()


_T = None


def tables():
    global _T
    if _T is None:
        _T = Tables()
    return _T


def lab2bgr(lab):
    """cv2.cvtColor(lab, COLOR_Lab2BGR) for uint8 (..., 3): Lab2RGBinteger::process per pixel."""
    t = tables()
    lab = np.asarray(lab, np.uint8)
    L, a, b = (lab[..., c].astype(np.int64) for c in range(3))
    y, ify = t.yf[L, 0], t.yf[L, 1]
    adiv = ((5 * a * 53687 + (1 << 7)) >> 13) - ADIV_BIAS
    bdiv = ((b * 41943 + (1 << 4)) >> 9) - BDIV_BIAS
    x = t.abxz[ify + adiv - MIN_AB]
    z = t.abxz[ify - bdiv - MIN_AB]
    out = np.empty(lab.shape, np.uint8)
    for c in range(3):
        v = (t.C[c, 0] * x + t.C[c, 1] * y + t.C[c, 2] * z + (1 << (DESCALE - 1))) >> DESCALE
        out[..., c] = t.invg[np.clip(v, 0, INV_GAMMA_TAB_SIZE - 1)]
    return out


def textbook_lab2bgr(lab):
    """Float64 CIE L*a*b* (D65) -> sRGB of 8-bit Lab (L* = 100 L / 255, a* = a - 128, b* = b - 128), scaled to [0, 255], unrounded."""
    lab = np.asarray(lab, np.float64)
    Ls, As, Bs = lab[..., 0] * (100.0 / 255.0), lab[..., 1] - 128.0, lab[..., 2] - 128.0
    fy = (Ls + 16.0) / 116.0
    fx, fz = fy + As / 500.0, fy - Bs / 200.0
    d = 6.0 / 29.0

    def finv(t):
        return np.where(t > d, t ** 3, 3 * d * d * (t - 4.0 / 29.0))
    X, Y, Z = WHITE[0] * finv(fx), finv(fy), WHITE[2] * finv(fz)
    out = np.empty(lab.shape, np.float64)
    for c, row in enumerate((XYZ2SRGB[2], XYZ2SRGB[1], XYZ2SRGB[0])):
        lin = np.clip(row[0] * X + row[1] * Y + row[2] * Z, 0.0, 1.0)
        out[..., c] = 255.0 * np.where(lin <= 0.0031308, 12.92 * lin, 1.055 * lin ** (1 / 2.4) - 0.055)
    return out


# ---- white balance ---------------------------------------------------------------------------------------------------------------------

NUMPY_CHUNK = 8192


def chunked_mean(plane_u8):
    """np.mean of plane.astype(float32) for a contiguous plane: float32 fold, from 0, of the exact sums of consecutive 8192-element
    chunks, divided by the count in binary64 and rounded to float32."""
    flat = np.ascontiguousarray(plane_u8).reshape(-1).astype(np.int64)
    acc = f32(0)
    for c0 in range(0, flat.size, NUMPY_CHUNK):
        acc = f32(acc + f32(int(flat[c0:c0 + NUMPY_CHUNK].sum())))
    return f32(float(acc) / float(flat.size))


def wrap_u8(v):
    """numpy's float32 -> uint8 astype for the values here: truncation toward zero, low 8 bits."""
    return (np.trunc(np.asarray(v, np.float32)).astype(np.int64) & 255).astype(np.uint8)


def box_mean(plane_u8, k):
    """cv2.blur(plane.astype(float32), (k, k), borderType=BORDER_REPLICATE): exact integer window sums (replicated border),
    float32(sum * (1.0 / (k * k)))."""
    p = np.asarray(plane_u8).astype(np.int64)
    h, w = p.shape
    r = k // 2
    rows = np.clip(np.arange(-r, h + r), 0, h - 1)
    cols = np.clip(np.arange(-r, w + r), 0, w - 1)
    ext = p[rows][:, cols]
    S = np.zeros((h + 2 * r + 1, w + 2 * r + 1), np.int64)
    S[1:, 1:] = ext.cumsum(0).cumsum(1)
    box = S[k:k + h, k:k + w] - S[:h, k:k + w] - S[k:k + h, :w] + S[:h, :w]
    return (box.astype(np.float64) * (1.0 / (k * k))).astype(np.float32)


def shifted_ab(lab_u8, a_avg, b_avg):
    """lab_a -= a_avg - 128 and the same for b, float32 throughout: (a', b') before the cast back to uint8."""
    a = lab_u8[..., 1].astype(np.float32) - (np.asarray(a_avg, np.float32) - np.float32(128))
    b = lab_u8[..., 2].astype(np.float32) - (np.asarray(b_avg, np.float32) - np.float32(128))
    return a, b


def white_balance_ab(lab_u8, kernel_size=None):
    """(a', b') of white_balance_bgr (kernel_size None) or of white_balance_bgr_blur: what the astype(np.uint8) wrap applies to."""
    if kernel_size is None:
        return shifted_ab(lab_u8, chunked_mean(lab_u8[..., 1]), chunked_mean(lab_u8[..., 2]))
    k = 2 * (kernel_size // 2) + 1
    return shifted_ab(lab_u8, box_mean(lab_u8[..., 1], k), box_mean(lab_u8[..., 2], k))


def _shift_planes(lab_u8, a_avg, b_avg):
    """shifted_ab, then astype(np.uint8) and LAB2BGR."""
    lab = lab_u8.copy()
    a, b = shifted_ab(lab_u8, a_avg, b_avg)
    lab[..., 1] = wrap_u8(a)
    lab[..., 2] = wrap_u8(b)
    return lab2bgr(lab)


def white_balance_bgr(lab_u8):
    """utils/color.py:370-378 given the 8-bit Lab image of the input; returns (bgr, (a_avg, b_avg))."""
    a_avg, b_avg = chunked_mean(lab_u8[..., 1]), chunked_mean(lab_u8[..., 2])
    return _shift_planes(lab_u8, a_avg, b_avg), (a_avg, b_avg)


def white_balance_bgr_blur(lab_u8, kernel_size):
    """utils/color.py:381-392 given the 8-bit Lab image of the input."""
    k = 2 * (kernel_size // 2) + 1
    if k <= 0:
        raise ValueError("kernel size")
    return _shift_planes(lab_u8, box_mean(lab_u8[..., 1], k), box_mean(lab_u8[..., 2], k))


def tie_margin(value):
    """Distance of `value` (a Fraction, float or mpmath number) from the nearest half-integer."""
    v = Fraction(value) if not isinstance(value, Fraction) else value
    frac = v - (v.numerator // v.denominator)
    return abs(frac - Fraction(1, 2))
