"""CPU statement of the Gaussian adaptive threshold: the float32 taps, the integer bounds the kernels rely on,
the restatement (adaptive_gauss_restate.py) against exact rational arithmetic, ties, the threshold rule and the facade's argument
errors, which are raised before anything is launched."""
from fractions import Fraction

import numpy as np
import pytest

import adaptive_gauss_restate as R

ODD = list(range(3, R.MAX_BLOCK + 1, 2))


def test_double_taps_far_from_float32_midpoints():
    # libm's exp against OpenCV's softdouble, and a fused against an unfused sigma, move a double tap by a few 2^-52 relative: a tap
    # this far from every float32 rounding midpoint rounds to the same float32 either way
    worst = 1.0
    for n in ODD:
        for fused in (False, True):
            k = R.kernel_f64(n, fused)
            for v in k[:n // 2 + 1]:
                f = np.float32(v)
                nb = (np.nextafter(f, np.float32(0)), np.nextafter(f, np.float32(1)))
                d = min(abs(Fraction(v) - (Fraction(float(f)) + Fraction(float(g))) / 2) for g in nb) / Fraction(float(f))
                worst = min(worst, float(d))
        assert np.array_equal(R.taps_f32(n), np.array(R.kernel_f64(n, True)).astype(np.float32)), n
    assert worst > 1e-12


def test_integer_bounds():
    # the kernels: t_i < 2^32, H = sum t p < 2^48 (pair sums S < 2^49 split at bit 24), A = sum t (S mod 2^24) and B = sum t (S >> 24)
    # below 2^64, the mean shift e_h + e_v <= 78
    es = []
    for n in [1] + ODD:
        t, e = R.int_taps(n)
        es.append(e)
        assert max(t) < 2**32 and sum(t) < 2**40
        assert t == t[::-1]
    assert max(es) == 39 and R.int_taps(1) == ([1], 0)
    # every (horizontal, vertical) pair of sizes: the largest pair sum against the largest vertical half-kernel sum bounds them all
    smax = max(2 * 255 * sum(R.int_taps(nh)[0]) for nh in [1] + ODD)
    half = max(sum(t[:len(t) // 2 + 1]) for t in (R.int_taps(nv)[0] for nv in [1] + ODD))
    assert smax < 2**56 and (smax >> 24) < 2**32
    assert ((1 << 24) - 1) * half < 2**64 and (smax >> 24) * half < 2**64


@pytest.mark.parametrize("n", [3, 5, 7, 9, 11, 13, 31, 51])
def test_restatement_equals_fractions(n):
    rng = np.random.default_rng(n)
    for h, w in ((6, 7), (1, 9), (9, 1), (1, 1), (4, 23), (3, 2)):
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        assert np.array_equal(R.gaussian_mean(img, n), R.fraction_mean(img, n)), (h, w)
    img = np.full((5, 5), 255, np.uint8)
    assert np.array_equal(R.gaussian_mean(img, n), R.fraction_mean(img, n))


def test_ties_round_to_even():
    # n = 3: taps 1/4, 1/2, 1/4, so the 2-D sum is an integer over 16; sums = 8 mod 16 are exact ties
    img = np.zeros((1, 1), np.uint8)
    for p in range(256):
        img[0, 0] = p
        assert R.gaussian_mean(img, 3)[0, 0] == p        # 1x1: the single tap 1.0 both ways
    # a 3-pixel row: mean of (a, b, c) with replicated ends = (a + 2b + c) / 4 along x, exact along y (h = 1)
    for a, b, c, exp in ((0, 0, 2, 0), (0, 1, 0, 0), (2, 1, 0, 1), (1, 1, 0, 1), (0, 1, 2, 1), (3, 0, 3, 2), (1, 0, 1, 0), (1, 1, 1, 1)):
        row = np.array([[a, b, c]], np.uint8)
        m = R.gaussian_mean(row, 3)[0, 1]
        assert m == exp and m == round(Fraction(a + 2 * b + c, 4)), (a, b, c)
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (40, 40), dtype=np.uint8)
    ref = R.fraction_mean(img[:8, :8], 3)
    assert np.array_equal(R.gaussian_mean(img[:8, :8], 3), ref)
    # a 2-D tie: sums = 8 mod 16
    img = np.zeros((3, 3), np.uint8)
    img[1, 1] = 2                                  # centre sum = 2 * 4 = 8 -> 8 / 16 = 0.5 -> 0
    assert R.gaussian_mean(img, 3)[1, 1] == 0
    img[1, 1] = 6                                  # 24 / 16 = 1.5 -> 2
    assert R.gaussian_mean(img, 3)[1, 1] == 2


def test_threshold_semantics():
    img = np.arange(256, dtype=np.uint8).reshape(16, 16)
    mean = np.full(img.shape, 100, np.uint8)
    out = R.apply_threshold(img, mean, 255, 0, 0)
    assert np.array_equal(out, np.where(img > 100, 255, 0))
    out = R.apply_threshold(img, mean, 255, 1, 0)
    assert np.array_equal(out, np.where(img <= 100, 255, 0))
    # idelta = ceil(C) for BINARY, floor(C) for BINARY_INV
    assert R.threshold_params(255, 0, 2.5) == (255, 3) and R.threshold_params(255, 1, 2.5) == (255, 2)
    assert R.threshold_params(255, 0, -2.5) == (255, -2) and R.threshold_params(255, 1, -2.5) == (255, -3)
    out = R.apply_threshold(img, mean, 255, 0, -2.5)
    assert np.array_equal(out, np.where(img.astype(int) - 100 > 2, 255, 0))
    out = R.apply_threshold(img, mean, 255, 1, 2.5)
    assert np.array_equal(out, np.where(img.astype(int) - 100 <= -2, 255, 0))
    # maxValue: rounded half to even, saturated; negative gives zeros
    assert R.threshold_params(200.4, 0, 0)[0] == 200 and R.threshold_params(200.5, 0, 0)[0] == 200
    assert R.threshold_params(201.5, 0, 0)[0] == 202 and R.threshold_params(300, 0, 0)[0] == 255 and R.threshold_params(0, 0, 0)[0] == 0
    assert not R.adaptive_threshold_gaussian(img, -1, 0, 3, 0).any()
    assert not R.adaptive_threshold_gaussian(img, -1, 1, 3, 0).any()


def test_thin_images_and_large_blocks():
    rng = np.random.default_rng(7)
    row = rng.integers(0, 256, (1, 97), dtype=np.uint8)
    col = row.reshape(97, 1)
    # one row: the vertical kernel is the single tap 1.0, so the mean is the horizontal pass alone (and likewise for one column)
    assert np.array_equal(R.gaussian_mean(row, 11).reshape(-1), R.gaussian_mean(col, 11).reshape(-1))
    t, e = R.int_taps(11)
    ref = [round(sum(Fraction(ti, 2**e) * int(row[0, min(max(x + i - 5, 0), 96)]) for i, ti in enumerate(t))) for x in range(97)]
    assert R.gaussian_mean(row, 11)[0].tolist() == [min(255, v) for v in ref]
    # a block larger than the image: replicated borders all the way
    img = rng.integers(0, 256, (5, 6), dtype=np.uint8)
    for n in (13, 31):
        assert np.array_equal(R.gaussian_mean(img, n), R.fraction_mean(img, n))
    big = rng.integers(0, 256, (9, 11), dtype=np.uint8)
    m = R.gaussian_mean(big, 511)
    assert m.shape == big.shape and m.dtype == np.uint8


def test_facade_argument_errors():
    from vision import cv2_facade as cv
    img = np.zeros((8, 8), np.uint8)
    cases = [
        (np.zeros((8, 8), np.float32), 255, cv.ADAPTIVE_THRESH_GAUSSIAN_C, cv.THRESH_BINARY, 3, 0),
        (np.zeros((8, 8, 3), np.uint8), 255, cv.ADAPTIVE_THRESH_GAUSSIAN_C, cv.THRESH_BINARY, 3, 0),
        (np.zeros((0, 8), np.uint8), 255, cv.ADAPTIVE_THRESH_GAUSSIAN_C, cv.THRESH_BINARY, 3, 0),
        (img, 255, cv.ADAPTIVE_THRESH_GAUSSIAN_C, cv.THRESH_BINARY, 4, 0),
        (img, 255, cv.ADAPTIVE_THRESH_GAUSSIAN_C, cv.THRESH_BINARY, 1, 0),
        (img, 255, cv.ADAPTIVE_THRESH_MEAN_C, cv.THRESH_BINARY, 0, 0),
        (img, 255, 2, cv.THRESH_BINARY, 3, 0),
        (img, 255, cv.ADAPTIVE_THRESH_GAUSSIAN_C, 2, 3, 0),
        (img, 255, cv.ADAPTIVE_THRESH_MEAN_C, 7, 3, 0),
    ]
    for args in cases:
        with pytest.raises(cv.error):
            cv.adaptiveThreshold(*args)
    assert (cv.ADAPTIVE_THRESH_MEAN_C, cv.ADAPTIVE_THRESH_GAUSSIAN_C, cv.THRESH_BINARY, cv.THRESH_BINARY_INV) == (0, 1, 0, 1)
    # thresh.cpp returns zeros for a negative maxValue before it looks at the method or the type
    assert not cv.adaptiveThreshold(img + 9, -1, 5, 9, 3, 0).any()

