"""Live comparison of tests/dist_restate.py with a real OpenCV's distanceTransform and minMaxLoc.  Skipped where `cv2` is not importable.
CPU-only.  The contract is cv2's own value wherever the image has a zero pixel - DIST_L2 with
DIST_MASK_PRECISE is the float32 root of an integer both sides compute, DIST_L1 and DIST_C are the integers the 3x3 chamfer computes - so
every comparison is exact.  The sizes stay at or below 640 x 480, well inside the widths for which section 4.25 argues that cv2's
float lower envelope picks the exact parabola.  An image without a zero pixel is left out: the declared deviation (section 7)."""
import numpy as np
import pytest

import dist_restate as R

cv2 = pytest.importorskip("cv2")
if not hasattr(cv2, "connectedComponentsWithStats") or getattr(cv2, "__name__", "") != "cv2" or "vision" in getattr(cv2, "__file__", ""):
    pytest.skip("the cv2 facade of this repo is not a reference", allow_module_level=True)


def _images():
    rng = np.random.default_rng(47)
    for h, w, density in ((1, 1, 1.0), (1, 37, 0.1), (41, 1, 0.1), (67, 35, 0.01), (67, 35, 0.5), (120, 160, 0.001), (480, 640, 0.0005), (480, 640, 0.3)):
        img = np.where(rng.random((h, w)) < density, 0, 255).astype(np.uint8)
        if img.all():
            img[h // 2, w // 3] = 0
        yield "random %dx%d at %g" % (w, h, density), img
    disc = np.zeros((240, 320), np.uint8)
    yy, xx = np.indices(disc.shape)
    disc[(yy - 100) ** 2 + (xx - 170) ** 2 <= 90 * 90] = 255
    disc[40:50, 10:300] = 200
    yield "disc and bar", disc
    corner = np.full((480, 640), 255, np.uint8)
    corner[479, 0] = 0
    yield "one zero in a corner", corner


def test_precise_l2_equals_cv2():
    for name, img in _images():
        ours = R.distance_transform(img, R.L2)
        theirs = cv2.distanceTransform(img, cv2.DIST_L2, cv2.DIST_MASK_PRECISE)
        assert theirs.dtype == np.float32 and ours.tobytes() == theirs.tobytes(), name


def test_l1_and_c_equal_cv2():
    for name, img in _images():
        for metric, code in ((R.L1, cv2.DIST_L1), (R.C, cv2.DIST_C)):
            for size in (3, 5, cv2.DIST_MASK_PRECISE):
                theirs = cv2.distanceTransform(img, code, size)
                assert R.distance_transform(img, metric).tobytes() == theirs.tobytes(), (name, metric, size)
        theirs = cv2.distanceTransform(img, cv2.DIST_L1, 3, dstType=cv2.CV_8U)
        assert theirs.dtype == np.uint8 and R.distance_transform(img, R.L1, np.uint8).tobytes() == theirs.tobytes(), name


def test_min_max_loc_equals_cv2():
    rng = np.random.default_rng(53)
    for h, w in ((1, 1), (1, 70), (33, 65), (480, 640)):
        mask = (rng.random((h, w)) < 0.5).astype(np.uint8) * 255
        for a in (rng.integers(3, 7, (h, w), dtype=np.uint8), (rng.integers(-2, 3, (h, w)) * 0.5).astype(np.float32)):
            assert R.min_max_loc(a) == tuple(cv2.minMaxLoc(a))
            assert R.min_max_loc(a, mask) == tuple(cv2.minMaxLoc(a, mask))
            assert R.min_max_loc(a, np.zeros_like(mask)) == tuple(cv2.minMaxLoc(a, np.zeros_like(mask)))
    f = np.array([[1.0, np.inf, -np.inf], [np.inf, -np.inf, 2.0]], np.float32)
    assert R.min_max_loc(f) == tuple(cv2.minMaxLoc(f))
    for name, img in _images():
        d = cv2.distanceTransform(img, cv2.DIST_L2, cv2.DIST_MASK_PRECISE)
        assert R.min_max_loc(d) == tuple(cv2.minMaxLoc(d)), name
