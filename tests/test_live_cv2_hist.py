"""Live comparison of tests/hist_restate.py with a real OpenCV's calcHist, calcBackProject and meanShift.  Skipped where `cv2` is not
importable.  CPU-only.  The contract is cv2's own value: the bin tables are calcHistLookupTables_8u's, the
counts and the back-projection integers, the mean-shift loop cv2's with exact sums - so every comparison is exact.  Left out: windows
with nothing of them inside the image (refused here, re-centred by cv2), products of hist and scale beyond the int range, normalize
and CamShift's box."""
import numpy as np
import pytest

import hist_restate as R

cv2 = pytest.importorskip("cv2")
if not hasattr(cv2, "connectedComponentsWithStats") or getattr(cv2, "__name__", "") != "cv2" or "vision" in getattr(cv2, "__file__", ""):
    pytest.skip("the cv2 facade of this repo is not a reference", allow_module_level=True)

CASES = (((0,), (180,), (0, 180)), ((0, 1), (180, 256), (0, 180, 0, 256)), ((2, 1), (7, 3), (10.5, 200.25, -20, 300)), ((0, 1, 2), (32, 32, 32), (0, 256) * 3),
         ((1,), (1,), (100, 101)), ((2, 0), (256, 5), (0, 256, 64, 65.5)))


def _image(h=67, w=83, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_calc_hist_equals_cv2():
    img = _image()
    mask = (np.random.default_rng(1).random(img.shape[:2]) < 0.6).astype(np.uint8) * 7
    for channels, sizes, ranges in CASES:
        for m in (None, mask):
            theirs = cv2.calcHist([img], list(channels), m, list(sizes), list(ranges))
            assert theirs.dtype == np.float32 and R.calc_hist(img, channels, sizes, ranges, m).tobytes() == theirs.reshape(sizes).tobytes(), (channels, sizes, ranges)


def test_back_project_equals_cv2():
    img = _image(seed=2)
    for channels, sizes, ranges in CASES:
        hist = R.normalize_hist(R.calc_hist(img[10:40, 20:60], channels, sizes, ranges), 255)
        for scale in (1.0, 0.5, 1.5, 20.0):
            theirs = cv2.calcBackProject([img], list(channels), hist, list(ranges), scale)
            assert theirs.dtype == np.uint8 and R.back_project(img, channels, hist, ranges, scale).tobytes() == theirs.tobytes(), (channels, sizes, scale)


def test_mean_shift_equals_cv2():
    yy, xx = np.mgrid[0:96, 0:128]
    prob = (255.0 * np.exp(-((xx - 80) ** 2 + (yy - 50) ** 2) / 400.0)).astype(np.uint8) + (np.random.default_rng(3).integers(0, 4, (96, 128))).astype(np.uint8)
    for window in ((60, 30, 20, 20), (0, 0, 128, 96), (70, 45, 1, 1), (-10, -10, 60, 70), (100, 70, 50, 50), (20, 20, 40, 9)):
        for kind, max_iter, eps in ((3, 10, 1.0), (1, 3, 0.0), (2, 0, 2.5), (3, 50, 0.4)):
            theirs = cv2.meanShift(prob, window, (kind, max_iter, eps))
            ours = R.mean_shift(prob, window, max_iter if kind & 1 else None, eps if kind & 2 else None)
            assert ours == (theirs[0], tuple(theirs[1])), (window, kind, max_iter, eps)
    assert R.mean_shift(np.zeros((9, 9), np.uint8), (2, 3, 4, 5), 10, 1.0) == (lambda r: (r[0], tuple(r[1])))(cv2.meanShift(np.zeros((9, 9), np.uint8), (2, 3, 4, 5), (3, 10, 1.0)))
