"""Independent numpy statement of cv2.adaptiveThreshold(src, maxValue, ADAPTIVE_THRESH_GAUSSIAN_C, type, blockSize, C) as this
project defines it: mean = the exact weighted mean of OpenCV's float32 taps getGaussianKernel(blockSize, 0,
CV_32F), separable, replicated borders, rounded half to even; then OpenCV's tab[src - mean + 255] compare.

The taps are computed here from OpenCV's recipe (getGaussianKernelBitExact: fixed tables for n = 3..9, the 0.15 n + 0.35 exp formula
otherwise) in Python double arithmetic and rounded to float32.  The exact sums are carried in uint64 limbs so that a 1080p frame
restates in seconds.  The product does not import this file."""
import math
from fractions import Fraction

import numpy as np

MAX_BLOCK = 511
_TABLES = {3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
           7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125],
           9: [v / 256.0 for v in (4, 13, 30, 51, 60, 51, 30, 13, 4)]}


def kernel_f64(n, fused=False):
    """getGaussianKernelBitExact(n, sigma=0) in doubles; fused: sigma = fma(n, 0.15, 0.35) (softdouble mulAdd) instead of n*0.15 + 0.35."""
    if n == 1:
        return [1.0]
    if n in _TABLES:
        return list(_TABLES[n])
    sx = float(Fraction(n) * Fraction(0.15) + Fraction(0.35)) if fused else n * 0.15 + 0.35
    scale2x = -0.125 / (sx * sx)
    n2 = (n - 1) // 2
    k = [0.0] * n
    s = 0.0
    for i in range(n2):
        x = 1 - n + 2 * i
        k[i] = math.exp(float(x * x) * scale2x)
        s += k[i]
    s = s * 2 + 1
    mul1 = 1.0 / s
    for i in range(n2):
        k[i] *= mul1
        k[n - 1 - i] = k[i]
    k[n2] = mul1
    return k


def taps_f32(n):
    return np.array(kernel_f64(n), np.float64).astype(np.float32)


def int_taps(n):
    """(t, e): the float32 taps as integers t_i * 2^-e, e the smallest exponent that makes every tap an integer."""
    fr = [Fraction(float(v)) for v in taps_f32(n)]
    e = 0
    for f in fr:
        d = f.denominator                      # a power of two
        e = max(e, d.bit_length() - 1)
    t = [int(f * 2**e) for f in fr]
    assert all(Fraction(ti, 2**e) == f for ti, f in zip(t, fr))
    return t, e


def _border_taps(block, w, h):
    """BORDER_ISOLATED: a one-pixel side takes the single tap 1.0 along that axis."""
    return int_taps(1 if w == 1 else block), int_taps(1 if h == 1 else block)


def gaussian_mean(img, block):
    """The exact Gaussian-weighted mean, rounded half to even and saturated to 255, as uint8 (h, w)."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    (th, eh), (tv, ev) = _border_taps(block, w, h)
    rh, rv = len(th) // 2, len(tv) // 2
    p = np.pad(img, ((0, 0), (rh, rh)), mode="edge").astype(np.uint64)
    H = np.zeros((h, w), np.uint64)
    for k, t in enumerate(th):                 # H < 255 * 2^40: exact in uint64
        H += np.uint64(t) * p[:, k:k + w]
    M = np.uint64((1 << 24) - 1)
    lo = np.pad(H & M, ((rv, rv), (0, 0)), mode="edge")
    hi = np.pad(H >> np.uint64(24), ((rv, rv), (0, 0)), mode="edge")
    A = np.zeros((h, w), np.uint64)
    B = np.zeros((h, w), np.uint64)
    for k, t in enumerate(tv):                 # A < 2^24 * sum(t) < 2^64, B < 255 * 2^(eh + ev - 24) (1 + 2^-20) < 2^63
        A += np.uint64(t) * lo[k:k + h]
        B += np.uint64(t) * hi[k:k + h]
    # V = A + B 2^24 = C 2^24 + a0
    C = B + (A >> np.uint64(24))
    a0 = A & M
    s = eh + ev
    if s >= 24:
        k = s - 24
        q = C >> np.uint64(k)
        if k == 0:
            above, tie = a0 > np.uint64(1 << 23), a0 == np.uint64(1 << 23)
        else:
            r = C & np.uint64((1 << k) - 1)
            half = np.uint64(1 << (k - 1))
            above = (r > half) | ((r == half) & (a0 > 0))
            tie = (r == half) & (a0 == 0)
    else:
        q = (C << np.uint64(24 - s)) + (a0 >> np.uint64(s))
        if s == 0:
            above = tie = np.zeros((h, w), bool)
        else:
            r = a0 & np.uint64((1 << s) - 1)
            half = np.uint64(1 << (s - 1))
            above, tie = r > half, r == half
    q = q + (above | (tie & ((q & np.uint64(1)) == 1))).astype(np.uint64)
    return np.minimum(q, 255).astype(np.uint8)


def fraction_mean(img, block):
    """The same mean by exact rational arithmetic, pixel by pixel (small images only)."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    th = [Fraction(float(v)) for v in taps_f32(1 if w == 1 else block)]
    tv = [Fraction(float(v)) for v in taps_f32(1 if h == 1 else block)]
    rh, rv = len(th) // 2, len(tv) // 2
    out = np.zeros((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            v = Fraction(0)
            for j, b in enumerate(tv):
                yy = min(max(y + j - rv, 0), h - 1)
                v += b * sum(a * int(img[yy, min(max(x + i - rh, 0), w - 1)]) for i, a in enumerate(th))
            out[y, x] = min(255, round(v))      # Python's round of a Fraction: half to even
    return out


def threshold_params(max_value, thresh_type, c):
    """(imax, idelta) of thresh.cpp: imaxval = saturate_cast<uchar>(maxValue) (round half to even), idelta = ceil(C) for BINARY,
    floor(C) for BINARY_INV."""
    imax = int(min(255, max(0, round(float(max_value)))))
    idelta = math.ceil(c) if thresh_type == 0 else math.floor(c)
    return imax, idelta


def apply_threshold(img, mean, max_value, thresh_type, c):
    img = np.asarray(img, np.uint8)
    if max_value < 0:
        return np.zeros(img.shape, np.uint8)
    imax, idelta = threshold_params(max_value, thresh_type, c)
    diff = img.astype(np.int32) - mean.astype(np.int32)
    on = diff > -idelta if thresh_type == 0 else diff <= -idelta
    return np.where(on, imax, 0).astype(np.uint8)


def adaptive_threshold_gaussian(img, max_value, thresh_type, block, c):
    img = np.asarray(img, np.uint8)
    if max_value < 0:
        return np.zeros(img.shape, np.uint8)
    return apply_threshold(img, gaussian_mean(img, block), max_value, thresh_type, c)
