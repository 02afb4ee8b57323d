"""Live comparison of the Hough statement (hough_restate.py) with a real OpenCV: what settles the open points of DESIGN.md (which
numangle rule, IPP) wherever cv2 exists.  Skipped where `cv2` is not importable (the build and GPU images).  CPU-only."""
import numpy as np
import pytest

import frames as F
import hough_restate as HR

cv2 = pytest.importorskip("cv2")
if not hasattr(cv2, "connectedComponentsWithStats") or getattr(cv2, "__name__", "") != "cv2" or "vision" in getattr(cv2, "__file__", ""):
    pytest.skip("the cv2 facade of this repo is not a reference", allow_module_level=True)


def _same(got, exp):
    if exp is None:
        assert got is None
    else:
        assert got is not None and got.shape == exp.shape and np.array_equal(got.view(np.uint32), exp.view(np.uint32))


@pytest.mark.parametrize("rho,theta,lo,hi", [(1, np.pi / 180, 0, np.pi), (0.5, np.pi / 360, 0, np.pi), (2, 0.3, 0, np.pi),
                                             (1, np.pi / 180, np.pi / 4, 3 * np.pi / 4)])
def test_statement_equals_cv2(rho, theta, lo, hi):
    rng = np.random.default_rng(0)
    edges = cv2.Canny(F.s2_bins(0, 320, 240)[:, :, 1].copy(), 40, 120)
    noise = ((rng.random((120, 160)) < 0.05) * 255).astype(np.uint8)
    for img in (edges, noise):
        for thr in (5, 40):
            _same(cv2.HoughLines(img, rho, theta, thr, None, 0, 0, lo, hi), HR.hough_lines(img, rho, theta, thr, lo, hi))
