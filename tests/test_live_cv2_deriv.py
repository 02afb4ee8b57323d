"""Live comparison of tests/deriv_restate.py with a real OpenCV's Sobel, Scharr, Laplacian, spatialGradient and convertScaleAbs at
scale = 1, delta = 0.  Skipped where `cv2` is not importable.  CPU-only."""
import numpy as np
import pytest

import deriv_restate as R

cv2 = pytest.importorskip("cv2")
if not hasattr(cv2, "connectedComponentsWithStats") or getattr(cv2, "__name__", "") != "cv2" or "vision" in getattr(cv2, "__file__", ""):
    pytest.skip("the cv2 facade of this repo is not a reference", allow_module_level=True)

SHAPES = [(1, 1, 1), (1, 9, 1), (9, 1, 1), (2, 2, 1), (3, 5, 1), (16, 512, 1), (17, 513, 1), (67, 35, 1), (67, 35, 3), (67, 35, 4), (301, 203, 3)]
BORDERS = [R.BORDER_REFLECT_101, R.BORDER_REPLICATE, R.BORDER_REFLECT, R.BORDER_CONSTANT]
DEPTHS = [-1, R.CV_16S, R.CV_32F, R.CV_64F]


def _images():
    rng = np.random.default_rng(4)
    for h, w, cn in SHAPES:
        yield rng.integers(0, 256, (h, w) if cn == 1 else (h, w, cn), dtype=np.uint8)
    step = np.zeros((40, 60), np.uint8)
    step[:, 30:] = 255
    yield step
    yield np.ascontiguousarray(step[:, ::-1])
    yield np.ascontiguousarray(step.T)


def _same(got, want):
    return got.dtype == want.dtype and np.array_equal(got.reshape(want.shape), want)


@pytest.mark.parametrize("border", BORDERS)
def test_cv2_sobel_scharr_laplacian_equal_the_restatement(border):
    for img in _images():
        for dd in DEPTHS:
            for k in (1, 3, 5, 7):
                for dx in range(3):
                    for dy in range(3):
                        if dx + dy > 0 and (k == 1 or max(dx, dy) < k):
                            assert _same(cv2.Sobel(img, dd, dx, dy, ksize=k, borderType=border), R.sobel_restate(img, dd, dx, dy, k, border)), (img.shape, dd, k, dx, dy)
                assert _same(cv2.Laplacian(img, dd, ksize=k, borderType=border), R.laplacian_restate(img, dd, k, border)), (img.shape, dd, k)
            for dx, dy in ((1, 0), (0, 1)):
                assert _same(cv2.Scharr(img, dd, dx, dy, borderType=border), R.scharr_restate(img, dd, dx, dy, border)), (img.shape, dd, dx, dy)
                assert _same(cv2.Sobel(img, dd, dx, dy, ksize=-1, borderType=border), R.scharr_restate(img, dd, dx, dy, border))


def test_cv2_spatial_gradient_and_rejections():
    for img in _images():
        if img.ndim != 2:
            continue
        for border in (R.BORDER_REFLECT_101, R.BORDER_REPLICATE):
            gx, gy = cv2.spatialGradient(img, ksize=3, borderType=border)
            ex, ey = R.spatial_gradient_restate(img, border)
            assert _same(gx, ex) and _same(gy, ey), (img.shape, border)
    g = np.zeros((6, 5), np.uint8)
    for call in (lambda: cv2.Sobel(g, cv2.CV_16S, 0, 0), lambda: cv2.Sobel(g, cv2.CV_16S, 3, 0, ksize=3), lambda: cv2.Sobel(g, cv2.CV_16S, 1, 0, borderType=cv2.BORDER_WRAP),
                 lambda: cv2.Scharr(g, cv2.CV_16S, 1, 1), lambda: cv2.spatialGradient(g, borderType=cv2.BORDER_REFLECT)):
        with pytest.raises(cv2.error):
            call()


def test_cv2_convert_scale_abs_equals_the_restatement():
    rng = np.random.default_rng(6)
    srcs = [np.array([[-32768, -32767, -256, -255, -254, -1, 0, 1, 254, 255, 256, 32767]], np.int16), rng.integers(-32768, 32768, (37, 29, 3)).astype(np.int16),
            np.array([[0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 253.5, 254.5, 255.5, -254.5, 0.49999997, 2.4999998, 1e6, -1e6]], np.float32),
            (rng.random((37, 29)) * 600 - 300).astype(np.float32), rng.random((37, 29)) * 600 - 300, rng.integers(0, 256, (37, 29, 4), dtype=np.uint8)]
    for src in srcs:
        assert _same(cv2.convertScaleAbs(src), R.convert_scale_abs_restate(src)), src.dtype
