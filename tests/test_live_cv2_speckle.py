"""Live comparison of tests/speckle_restate.py with a real OpenCV's cv2.filterSpeckles: the differing pixels are reported per case.
Skipped where `cv2` is not importable.  CPU-only.

No machine this library was built on has had `cv2`: the restatement follows the documented rule of filterSpeckles (4-neighbours, the
difference taken against the pixel just popped, regions of at most maxSpeckleSize pixels replaced), and parity with cv2's bytes is
not claimed (DESIGN.md sections 4.35 and 7).  If a pixel ever differs, the rule to revisit is the statement's - whether the limit is
inclusive, whether new_val pixels separate regions - and not the kernel, which is pinned to the statement byte for byte by
tests/test_gpu_speckle.py."""
import numpy as np
import pytest

import speckle_cases as SC
import speckle_restate as R

cv2 = pytest.importorskip("cv2")
if not hasattr(cv2, "connectedComponentsWithStats") or getattr(cv2, "__name__", "") != "cv2" or "vision" in getattr(cv2, "__file__", ""):
    pytest.skip("the cv2 facade of this repo is not a reference", allow_module_level=True)

CASES = SC.cases(32)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_pixels_that_differ_from_cv2(case):
    img = case["image"]()
    got = img.copy()
    cv2.filterSpeckles(got, case["new_val"], case["max_size"], case["max_diff"])
    want = R.filter_speckles(img, case["new_val"], case["max_size"], case["max_diff"])
    assert got.dtype == np.int16 and got.shape == want.shape
    differ = np.argwhere(got != want)
    print(f"filterSpeckles {case['id']}: {len(differ)} of {img.size} pixels differ" + (f", the first at (y, x) = {tuple(differ[0])}" if len(differ) else ""))
