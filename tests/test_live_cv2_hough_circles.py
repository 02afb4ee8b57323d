"""Live comparison of the HoughCircles statement (hough_circles_restate.py) with a real OpenCV: what settles the open points A-C of
DESIGN.md section 4.13 (the centre's border cell, the rounding of param1 / param2, the point-mask form of the radius filter) wherever cv2
exists.  Skipped where `cv2` is not importable (the build and GPU images).  CPU-only."""
import numpy as np
import pytest

import frames as F
import hough_circles_restate as HC
from test_hough_circles_statement import discs

cv2 = pytest.importorskip("cv2")
if not hasattr(cv2, "connectedComponentsWithStats") or getattr(cv2, "__name__", "") != "cv2" or "vision" in getattr(cv2, "__file__", ""):
    pytest.skip("the cv2 facade of this repo is not a reference", allow_module_level=True)


def _same(got, exp):
    if exp is None:
        assert got is None
    else:
        assert got is not None and got.shape == exp.shape and np.array_equal(got.view(np.uint32), exp.view(np.uint32))


@pytest.mark.parametrize("dp,md,p1,p2,rmin,rmax", [(1, 20, 100, 20, 0, 0), (1.5, 10, 80, 15, 5, 60), (2, 30, 100, 12, 0, 90),
                                                   (1, 20, 100.5, 20.5, 10, 40), (1, 5, 100, 8, 3, 30)])
def test_statement_equals_cv2(dp, md, p1, p2, rmin, rmax):
    imgs = [np.ascontiguousarray(F.s1_buoy(0, 320, 240)[:, :, 1]), np.ascontiguousarray(F.s2_bins(1, 320, 240)[:, :, 1]),
            discs(1, 240, 320, ((80, 70, 30), (220, 150, 45), (270, 50, 18)))]
    for img in imgs:
        _same(cv2.HoughCircles(img, cv2.HOUGH_GRADIENT, dp, md, None, p1, p2, rmin, rmax),
              HC.hough_circles(img, dp, md, p1, p2, rmin, rmax, canny=cv2.Canny))
