"""Live comparison of tests/clahe_restate.py with a real OpenCV's equalizeHist and createCLAHE(...).apply on the small cases of the
GPU suite, the padding-quirk case and the rounding-tie case among them.  Skipped where `cv2` is not importable.  CPU-only."""
import numpy as np
import pytest

import clahe_restate as R

cv2 = pytest.importorskip("cv2")
if not hasattr(cv2, "connectedComponentsWithStats") or getattr(cv2, "__name__", "") != "cv2" or "vision" in getattr(cv2, "__file__", ""):
    pytest.skip("the cv2 facade of this repo is not a reference", allow_module_level=True)

CLIPS = [0, 1e-3, 2.0, 40.0, 1e4]
CASES = [((64, 64), (8, 8)), ((16, 16), (8, 8)), ((37, 29), (4, 3)), ((40, 29), (4, 3)), ((37, 30), (4, 3)), ((9, 9), (8, 8)), ((61, 45), (1, 1)), ((61, 45), (1, 8)),
         ((61, 45), (8, 1)), ((256, 192), (2, 2)), ((85, 64), (17, 16))]


def _images(w, h):
    rng = np.random.default_rng(w * 1009 + h)
    yield rng.integers(0, 256, (h, w), dtype=np.uint8)
    yield rng.integers(90, 99, (h, w), dtype=np.uint8)
    yield np.full((h, w), 131, np.uint8)
    yield np.where(rng.random((h, w)) < 0.3, 200, 17).astype(np.uint8)


@pytest.mark.parametrize("size,grid", CASES)
def test_cv2_clahe_equals_the_restatement(size, grid):
    for img in _images(*size):
        for clip in CLIPS:
            got = cv2.createCLAHE(clipLimit=clip, tileGridSize=grid).apply(img)
            assert got.dtype == np.uint8 and np.array_equal(got, R.clahe(img, clip, grid)), (size, grid, clip)


@pytest.mark.parametrize("size", [s for s, _ in CASES])
def test_cv2_equalize_hist_equals_the_restatement(size):
    for img in _images(*size):
        assert np.array_equal(cv2.equalizeHist(img), R.equalize_hist(img)), size
    for v in (0, 9, 255):
        img = np.full((size[1], size[0]), v, np.uint8)
        assert np.array_equal(cv2.equalizeHist(img), R.equalize_hist(img))


def test_cv2_defaults_are_the_facades():
    c = cv2.createCLAHE()
    assert c.getClipLimit() == 40.0 and tuple(c.getTilesGridSize()) == (8, 8)
