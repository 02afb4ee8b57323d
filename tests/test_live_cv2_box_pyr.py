"""Live comparison of tests/box_pyr_restate.py with a real OpenCV's boxFilter, blur, pyrDown, pyrUp and integral.  Skipped where `cv2`
is not importable.  CPU-only.  A disagreement here is a failure of the statement, not of the kernels."""
import numpy as np
import pytest

import box_pyr_restate as R

cv2 = pytest.importorskip("cv2")
if not hasattr(cv2, "connectedComponentsWithStats") or getattr(cv2, "__name__", "") != "cv2" or "vision" in getattr(cv2, "__file__", ""):
    pytest.skip("the cv2 facade of this repo is not a reference", allow_module_level=True)

SHAPES = [(1, 1, 1), (1, 9, 1), (9, 1, 1), (2, 2, 1), (3, 5, 1), (32, 256, 1), (33, 257, 1), (67, 35, 1), (67, 35, 3), (67, 35, 4), (301, 203, 3)]
WINDOWS = [(1, 1), (3, 3), (2, 2), (4, 3), (5, 1), (1, 7), (15, 15), (151, 151)]


def _images():
    rng = np.random.default_rng(4)
    for h, w, cn in SHAPES:
        yield rng.integers(0, 256, (h, w) if cn == 1 else (h, w, cn), dtype=np.uint8)
    yield np.full((67, 35), 255, np.uint8)


def _same(got, want):
    return got.dtype == want.dtype and np.array_equal(got.reshape(want.shape), want)


def test_statement_equals_cv2_box_filter():
    for img in _images():
        for kw, kh in WINDOWS:
            for border in R.BOX_BORDERS:
                for dd in (-1, R.CV_16S, R.CV_32S, R.CV_32F, R.CV_64F):
                    want = cv2.boxFilter(img, dd, (kw, kh), normalize=False, borderType=border)
                    assert _same(R.box_filter_restate(img, dd, kw, kh, False, border), want), (img.shape, kw, kh, border, dd)
                if R.area_is_exact(kw * kh):
                    assert _same(R.box_filter_restate(img, -1, kw, kh, True, border), cv2.blur(img, (kw, kh), borderType=border)), (img.shape, kw, kh, border)


def test_statement_equals_cv2_pyramids_and_integral():
    for img in _images():
        for border in R.PYR_DOWN_BORDERS:
            assert _same(R.pyr_down_restate(img, border), cv2.pyrDown(img, borderType=border)), (img.shape, border)
        assert _same(R.pyr_up_restate(img), cv2.pyrUp(img)), img.shape
        assert _same(R.integral_restate(img), cv2.integral(img)), img.shape
