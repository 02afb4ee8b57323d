"""Live comparison of the Gaussian adaptive-threshold statement (adaptive_gauss_restate.py) with a real OpenCV: what settles the open
points of DESIGN.md section 4.11 (how far a build's float32 blur strays from the exact mean, the one-row / one-column rule) wherever
cv2 exists.  Skipped where `cv2` is not importable (the build and GPU images).  CPU-only."""
from fractions import Fraction

import numpy as np
import pytest

import adaptive_gauss_restate as R

cv2 = pytest.importorskip("cv2")
if not hasattr(cv2, "connectedComponentsWithStats") or getattr(cv2, "__name__", "") != "cv2" or "vision" in getattr(cv2, "__file__", ""):
    pytest.skip("the cv2 facade of this repo is not a reference", allow_module_level=True)


def _exact_means(img, block, ys, xs):
    h, w = img.shape
    th = [Fraction(float(v)) for v in R.taps_f32(1 if w == 1 else block)]
    tv = [Fraction(float(v)) for v in R.taps_f32(1 if h == 1 else block)]
    rh, rv = len(th) // 2, len(tv) // 2
    out = []
    for y, x in zip(ys, xs):
        v = Fraction(0)
        for j, b in enumerate(tv):
            yy = min(max(y + j - rv, 0), h - 1)
            v += b * sum(a * int(img[yy, min(max(x + i - rh, 0), w - 1)]) for i, a in enumerate(th))
        out.append(v)
    return out


@pytest.mark.parametrize("block", [3, 5, 11, 31, 151])
def test_differences_lie_at_half_integers(block):
    rng = np.random.default_rng(block)
    img = rng.integers(0, 256, (120, 160), dtype=np.uint8)
    mean = R.gaussian_mean(img, block)
    for ttype in (cv2.THRESH_BINARY, cv2.THRESH_BINARY_INV):
        for c in (0, 2.5, -3):
            got = cv2.adaptiveThreshold(img, 255, cv2.ADAPTIVE_THRESH_GAUSSIAN_C, ttype, block, c)
            exp = R.apply_threshold(img, mean, 255, ttype, c)
            ys, xs = np.nonzero(got != exp)
            # a pixel may differ only where the exact mean lies within cv2's float32 error of a half-integer.  Each pass sums n
            # products of taps (sum about 1) and values <= 255 in float32; a sum of n terms has an error of at most about
            # n * 2^-24 * 255, and the products, the second pass's inherited error and the final rounding add a few more units.
            # Bound: (2 n + 4) * 2^-24 * 256 = (2 n + 4) * 2^-16.
            tol = Fraction(2 * block + 4, 1 << 16)
            for v in _exact_means(img, block, ys[:200], xs[:200]):
                frac = v - int(v)
                assert abs(frac - Fraction(1, 2)) <= tol, (float(v), block)


@pytest.mark.parametrize("shape", [(1, 97), (97, 1), (1, 1)])
def test_one_row_and_one_column_rule(shape):
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    for block in (3, 11, 31):
        got = cv2.adaptiveThreshold(img, 255, cv2.ADAPTIVE_THRESH_GAUSSIAN_C, cv2.THRESH_BINARY, block, 0)
        exp = R.adaptive_threshold_gaussian(img, 255, 0, block, 0)
        assert np.array_equal(got, exp), (shape, block)
