"""Live comparison of tests/moments_restate.py with a real OpenCV's moments and HuMoments.  Skipped where `cv2` is not importable.
CPU-only.  A disagreement here is a failure of the statement, not of the kernels."""
import numpy as np
import pytest

import moments_restate as R

cv2 = pytest.importorskip("cv2")
if not hasattr(cv2, "connectedComponentsWithStats") or getattr(cv2, "__name__", "") != "cv2" or "vision" in getattr(cv2, "__file__", ""):
    pytest.skip("the cv2 facade of this repo is not a reference", allow_module_level=True)


def _fields(m):
    assert list(m) == list(R.FIELDS)
    return R.as_bytes([m[k] for k in R.FIELDS])


def _contours():
    rng = np.random.default_rng(23)
    for n in (3, 4, 7, 64, 500):
        yield rng.integers(0, 32768, (n, 1, 2)).astype(np.int32)
        yield (rng.random((n, 1, 2)) * 2000 - 300).astype(np.float32)
    yield np.array([[[5, 7]]], np.int32)
    yield np.array([[[5, 7]], [[9, 2]]], np.int32)
    yield np.array([[[0, 0]], [[0, 5]], [[6, 5]], [[6, 0]]], np.int32)
    yield np.array([[[0, 0]], [[6, 0]], [[6, 5]], [[0, 5]]], np.int32)


def test_statement_equals_cv2_contour_moments_and_hu():
    for c in _contours():
        m = cv2.moments(c)
        exp = R.complete(R.contour_moments(c))
        assert _fields(m) == R.as_bytes(exp), (c.dtype, len(c))
        assert cv2.HuMoments(m).tobytes() == R.as_bytes(R.hu(exp)), (c.dtype, len(c))


def test_statement_equals_cv2_raster_moments_below_2_53():
    rng = np.random.default_rng(4)
    images = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((1, 1), (1, 9), (9, 1), (2, 2), (67, 35), (301, 203), (40, 1025))]
    images += [rng.choice(np.array([0, 3, 255], np.uint8), (67, 35)), np.zeros((5, 5), np.uint8), np.full((2, 2100), 255, np.uint8),
               (rng.random((1080, 1920)) < 0.3).astype(np.uint8) * 255]
    for img in images:
        for binary in (False, True):
            sums = R.raster_moments(img, binary)
            if max(sums) >= 2 ** 53:
                continue                        # above it OpenCV's last bits depend on its tile order
            m = cv2.moments(img, binaryImage=binary)
            exp = R.complete(sums)
            assert _fields(m) == R.as_bytes(exp), (img.shape, binary)
            assert cv2.HuMoments(m).tobytes() == R.as_bytes(R.hu(exp)), (img.shape, binary)
