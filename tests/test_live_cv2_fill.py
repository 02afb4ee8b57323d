"""Live comparison of the fill statement (fill_restate.py: even-odd scanline, then the outline) with a real OpenCV's
cv2.drawContours(..., thickness=-1).  Equality is claimed - and asserted - for one class of input only: the contours cv2.findContours
produces for blobs (what fill_ratio, vision_common.py:282-288, fills).  For arbitrary polygons the two rasterisers are compared and the
count of differing cases is printed, not asserted.  Skipped where `cv2` is not importable (the build and GPU images).  CPU-only."""
import numpy as np
import pytest

import fill_restate as R

cv2 = pytest.importorskip("cv2")
if not hasattr(cv2, "connectedComponentsWithStats") or getattr(cv2, "__name__", "") != "cv2" or "vision" in getattr(cv2, "__file__", ""):
    pytest.skip("the cv2 facade of this repo is not a reference", allow_module_level=True)


def _blobs(seed, h=96, w=128):
    """A random mask of a few overlapping discs and boxes with holes punched in."""
    rng = np.random.default_rng(seed)
    m = np.zeros((h, w), np.uint8)
    yy, xx = np.mgrid[:h, :w]
    for _ in range(int(rng.integers(2, 6))):
        cx, cy, r = int(rng.integers(0, w)), int(rng.integers(0, h)), int(rng.integers(3, 25))
        if rng.random() < 0.5:
            m[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 255
        else:
            m[max(cy - r, 0):cy + r, max(cx - r // 2, 0):cx + r // 2] = 255
    for _ in range(int(rng.integers(0, 4))):
        cx, cy, r = int(rng.integers(0, w)), int(rng.integers(0, h)), int(rng.integers(1, 6))
        m[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 0
    return m


@pytest.mark.parametrize("method", ["CHAIN_APPROX_SIMPLE", "CHAIN_APPROX_NONE"])
def test_contours_of_blobs_fill_as_cv2_does(method):
    differing = []
    for seed in range(40):
        m = _blobs(seed)
        contours = cv2.findContours(m, cv2.RETR_LIST, getattr(cv2, method))[-2]
        for k, c in enumerate(contours):
            want = np.zeros_like(m)
            cv2.drawContours(want, [c], -1, 255, thickness=-1)
            got = np.zeros_like(m)
            R.statement(got, [c], np.uint8(255))
            if not np.array_equal(got, want):
                differing.append((seed, k, int((got != want).sum())))
    print(f"{method}: contours whose fill differs from cv2: {differing}")
    assert not differing


def test_arbitrary_polygons_are_reported():
    rng = np.random.default_rng(0)
    total = differing = 0
    for name, polys in R.CASES.items():
        for p in polys:
            want, got = np.zeros((110, 200), np.uint8), np.zeros((110, 200), np.uint8)
            cv2.drawContours(want, [np.asarray(p, np.int32).reshape(-1, 1, 2)], -1, 255, thickness=-1)
            R.statement(got, [p], np.uint8(255))
            total += 1
            differing += int(not np.array_equal(got, want))
    for _ in range(100):
        p = rng.integers(-20, 220, (int(rng.integers(3, 9)), 2)).astype(np.int32)
        want, got = np.zeros((110, 200), np.uint8), np.zeros((110, 200), np.uint8)
        cv2.drawContours(want, [p.reshape(-1, 1, 2)], -1, 255, thickness=-1)
        R.statement(got, [p], np.uint8(255))
        total += 1
        differing += int(not np.array_equal(got, want))
    print(f"arbitrary polygons: {differing} of {total} differ from cv2 (reported, not asserted)")
