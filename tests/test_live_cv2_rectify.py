"""Live comparison of vision.utils.stereo.stereo_rectify with a real OpenCV's cv2.stereoRectify: the differences are reported per rig, not
asserted.  Skipped where `cv2` is not importable.  CPU-only.

No machine this library was built on has had `cv2`: the statement follows Bouguet's published algorithm step by step and parity with
cv2's numbers is not claimed (DESIGN.md sections 4.37 and 7).  What must hold whatever cv2 says is in tests/test_rectify_statement.py.
If the rotations ever differ, the rule to revisit is the choice of the axis; if only the projections do, the focal length (this
statement takes the mean of the two cameras'), the corners that centre the principal points, or the alpha scale."""
import numpy as np
import pytest

from test_rectify_statement import SIZE, _rig

cv2 = pytest.importorskip("cv2")
if not hasattr(cv2, "connectedComponentsWithStats") or getattr(cv2, "__name__", "") != "cv2" or "vision" in getattr(cv2, "__file__", ""):
    pytest.skip("the cv2 facade of this repo is not a reference", allow_module_level=True)


@pytest.mark.parametrize("name", ["horizontal", "vertical", "identity"])
@pytest.mark.parametrize("alpha", [-1, 0, 1])
def test_differences_from_cv2(name, alpha):
    from vision.utils import stereo
    K1, d1, K2, d2, R, T = _rig(name)
    zeros = np.zeros(5)
    got = stereo.stereo_rectify(K1, d1, K2, d2, SIZE, R, T, alpha=alpha)
    want = cv2.stereoRectify(K1, zeros if d1 is None else np.asarray(d1, float), K2, zeros if d2 is None else np.asarray(d2, float), SIZE, R, T.reshape(3, 1),
                             flags=cv2.CALIB_ZERO_DISPARITY, alpha=alpha)
    names = ("R1", "R2", "P1", "P2", "Q")
    print(f"{name} alpha={alpha}: " + ", ".join(f"max |{n} - cv2| = {np.abs(np.asarray(a) - np.asarray(b)).max():.3g}" for n, a, b in zip(names, got, want))
          + f"; roi1 {got[5]} against {tuple(want[5])}, roi2 {got[6]} against {tuple(want[6])}")
    assert all(np.asarray(a).shape == np.asarray(b).shape for a, b in zip(got[:5], want[:5]))
