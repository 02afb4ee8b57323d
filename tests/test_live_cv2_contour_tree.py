"""Live comparison of the RETR_CCOMP / RETR_TREE statement (contour_tree_restate.py, statement (a)) with a real OpenCV: what settles
the order of siblings and the parent rule wherever cv2 exists.  Skipped where `cv2` is not importable (the build and GPU images).
CPU-only."""
import numpy as np
import pytest

import contour_tree_restate as R
import frames as F

cv2 = pytest.importorskip("cv2")
if not hasattr(cv2, "connectedComponentsWithStats") or getattr(cv2, "__name__", "") != "cv2" or "vision" in getattr(cv2, "__file__", ""):
    pytest.skip("the cv2 facade of this repo is not a reference", allow_module_level=True)


@pytest.mark.parametrize("mode", [R.RETR_CCOMP, R.RETR_TREE])
@pytest.mark.parametrize("method", [cv2.CHAIN_APPROX_NONE, cv2.CHAIN_APPROX_SIMPLE])
def test_statement_equals_cv2(mode, method):
    rng = np.random.default_rng(17)
    for trial in range(200):
        m = F.random_mask(rng, int(rng.integers(1, 40)), int(rng.integers(1, 60)))
        cs, hier = cv2.findContours(m.copy(), mode, method)
        lst, _ = cv2.findContours(m.copy(), cv2.RETR_LIST, method)
        exp, _, eh = R.expected(m, mode, list(lst))
        assert len(cs) == len(exp)
        assert all(np.array_equal(a, b) for a, b in zip(cs, exp))
        if len(exp):
            assert np.array_equal(hier[0], eh)
        else:
            assert hier is None
