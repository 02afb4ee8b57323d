"""Live comparison of tests/stereo_restate.py with a real OpenCV's cv2.StereoBM, inside cv2's own getValidDisparityROI only: the share of
differing pixels is reported per case.  Skipped where `cv2` is not importable.  CPU-only.

No machine this library was built on has had `cv2`: the restatement follows the published design of StereoBM step by step, and parity
with cv2's bits is not claimed (DESIGN.md sections 4.34 and 7).  If the interior ever differs, the rule to revisit is the tie order of
the minimum, the row reflection of the prefilter or the mirrored cost at an end of the disparity range - rules of the statement - and
not the kernel, which is pinned to the statement byte for byte by tests/test_gpu_stereo.py."""
import numpy as np
import pytest

import stereo_cases as SC
import stereo_restate as R

cv2 = pytest.importorskip("cv2")
if not hasattr(cv2, "connectedComponentsWithStats") or getattr(cv2, "__name__", "") != "cv2" or "vision" in getattr(cv2, "__file__", ""):
    pytest.skip("the cv2 facade of this repo is not a reference", allow_module_level=True)


@pytest.mark.parametrize("n,bs,pair", [(16, 9, "planes"), (32, 15, "shift"), (64, 21, "shift"), (16, 5, "noisy")])
def test_share_of_pixels_that_differ_inside_cv2s_valid_roi(n, bs, pair):
    left, right = {"planes": lambda: SC.two_plane_pair(60, 240, 7), "shift": lambda: SC.shifted_pair(80, 320, 9, 4),
                   "noisy": lambda: SC.shifted_pair(60, 240, 6, 8, noise=40)}[pair]()
    h, w = left.shape
    bm = cv2.StereoBM_create(n, bs)
    got = bm.compute(left, right)
    want = R.disparity(left, right, num_disparities=n, block_size=bs, min_disparity=bm.getMinDisparity(), pre_filter_cap=bm.getPreFilterCap(),
                       texture_threshold=bm.getTextureThreshold(), uniqueness_ratio=bm.getUniquenessRatio())
    x, y, rw, rh = cv2.getValidDisparityROI((0, 0, w, h), (0, 0, w, h), bm.getMinDisparity(), n, bs)
    assert rw > 0 and rh > 0 and got.dtype == np.int16 and got.shape == want.shape
    a, b = got[y:y + rh, x:x + rw], want[y:y + rh, x:x + rw]
    share = float((a != b).mean())
    print(f"StereoBM n={n} block={bs} {pair}: valid ROI {(x, y, rw, rh)} against the statement's {R.valid_rect(w, h, n, bs, bm.getMinDisparity())}; "
          f"{share:.4%} of {a.size} pixels differ (largest difference {int(np.abs(a.astype(np.int32) - b).max())} sixteenths)")
