"""Live comparison of tests/median_restate.py with a real OpenCV's cv2.medianBlur, and cv2's own answer to the one point of the
stand-in that was written from memory of OpenCV's source: two channels with a window above 5 (the point marked
there).  Skipped where `cv2` is not importable.  CPU-only."""
import numpy as np
import pytest

from median_restate import median_restate

cv2 = pytest.importorskip("cv2")
if not hasattr(cv2, "connectedComponentsWithStats") or getattr(cv2, "__name__", "") != "cv2" or "vision" in getattr(cv2, "__file__", ""):
    pytest.skip("the cv2 facade of this repo is not a reference", allow_module_level=True)

SHAPES = [(1, 1), (1, 7), (7, 1), (2, 3), (5, 4), (37, 29), (77, 300), (300, 77)]


@pytest.mark.parametrize("k", [3, 5, 7, 15])
def test_cv2_medianblur_equals_the_restatement(k):
    rng = np.random.default_rng(k)
    for (h, w) in SHAPES:
        for cn in (1, 3, 4):
            for img in (rng.integers(0, 256, (h, w, cn), dtype=np.uint8), rng.choice(np.array([0, 1, 254, 255], np.uint8), (h, w, cn)),
                        np.where(rng.random((h, w, cn)) < 0.1, 255, 0).astype(np.uint8)):
                img = np.ascontiguousarray(img[:, :, 0]) if cn == 1 else img
                got = cv2.medianBlur(img, k)
                assert np.array_equal(got.reshape(img.shape), median_restate(img, k)), (h, w, cn, k)


def test_cv2_two_channels():
    """3 and 5 are served for two channels; what cv2 says to 7 is recorded (the stand-in raises: cv2 asserts 1, 3 or 4 channels there)"""
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (37, 29, 2), dtype=np.uint8)
    for k in (3, 5):
        assert np.array_equal(cv2.medianBlur(img, k), median_restate(img, k)), k
    try:
        got = cv2.medianBlur(img, 7)
    except cv2.error as e:
        print("cv2.medianBlur, 2 channels, ksize 7: raises", str(e).strip().splitlines()[-1])
        return
    same = np.array_equal(got, median_restate(img, 7))
    print("cv2.medianBlur, 2 channels, ksize 7: returns a result; equal to the restatement:", same)
    assert same, "cv2 serves two channels above 5 and differs from the restatement: the stand-in's rejection and DESIGN.md 4.18 need a look"
