"""Live comparison of tests/flow_restate.py with a real OpenCV's calcOpticalFlowPyrLK.  Opt-in: skipped where `cv2` is not importable.
CPU-only.  The contract is the exact value of what cv2's float32 SIMD code approximates, not its bits: status
must agree wherever the point is not at a threshold, and positions agree within a tolerance that has to be measured against the cv2
at hand.  No OpenCV has been met yet: the tolerance below is reasoned, not measured - cv2 accumulates at most
63 * 63 float32 products per sum (relative error about 4000 * 2^-24 = 2.4e-4 of A and b), which moves a converged position by far
less than the 0.01-pixel stopping rule does, so positions are compared at 0.05 pixels - five stopping steps."""
import numpy as np
import pytest

import flow_restate as R

cv2 = pytest.importorskip("cv2")
if not hasattr(cv2, "connectedComponentsWithStats") or getattr(cv2, "__name__", "") != "cv2" or "vision" in getattr(cv2, "__file__", ""):
    pytest.skip("the cv2 facade of this repo is not a reference", allow_module_level=True)

POSITION_TOLERANCE = 0.05


@pytest.mark.parametrize("win,max_level", [((21, 21), 3), ((21, 21), 0), ((9, 13), 2), ((31, 15), 1)])
def test_status_and_positions_follow_cv2(win, max_level):
    shift = (2.3, -1.6)
    a, b = R.texture(120, 160, 1), R.texture(120, 160, 1, shift)
    ys, xs = np.mgrid[6:114:9, 6:154:9]
    pts = np.stack([xs.ravel() + 0.25, ys.ravel() + 0.5], 1).astype(np.float32)
    theirs, st, err = cv2.calcOpticalFlowPyrLK(a, b, pts.reshape(-1, 1, 2), None, winSize=win, maxLevel=max_level,
                                               criteria=(cv2.TERM_CRITERIA_COUNT | cv2.TERM_CRITERIA_EPS, 30, 0.01))
    ours, ok, e = R.lk_restate(a, b, pts, win=win, max_level=max_level)
    st = st.ravel() != 0
    print("status differs at", int((st != (ok != 0)).sum()), "of", len(pts))
    both = st & (ok != 0)
    d = np.abs(theirs.reshape(-1, 2)[both] - ours[both])
    print("worst position difference", float(d.max()), "worst err difference", float(np.abs(err.ravel()[both] - e[both]).max()))
    assert (st == (ok != 0)).mean() > 0.98, "status may differ only for points at a threshold"
    assert d.max() <= POSITION_TOLERANCE
