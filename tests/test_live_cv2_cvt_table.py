"""Live comparison of the restatement of the added colour conversions (cvt_table_restate.py) with a real OpenCV, wherever `cv2` is
importable (not on the build and GPU images: skipped there).  CPU-only.  The constants of the restatement are written from memory of
OpenCV 4.x; this file is what pins them."""
import numpy as np
import pytest

import cvt_table_restate as R

cv2 = pytest.importorskip("cv2")
if not hasattr(cv2, "connectedComponentsWithStats") or getattr(cv2, "__name__", "") != "cv2" or "vision" in getattr(cv2, "__file__", ""):
    pytest.skip("the cv2 facade of this repo is not a reference", allow_module_level=True)

CV_NAMES = {"BGR2YUV": "BGR2YUV", "YUV2BGR": "YUV2BGR", "YCRCB2BGR": "YCrCb2BGR", "BGR2XYZ": "BGR2XYZ", "XYZ2BGR": "XYZ2BGR", "HLS2BGR": "HLS2BGR",
            "BGR2RGB": "BGR2RGB", "RGB2YUV": "RGB2YUV", "YUV2RGB": "YUV2RGB", "RGB2YCRCB": "RGB2YCrCb", "YCRCB2RGB": "YCrCb2RGB",
            "RGB2XYZ": "RGB2XYZ", "XYZ2RGB": "XYZ2RGB", "HLS2RGB": "HLS2RGB", "RGB2GRAY": "RGB2GRAY", "BGRA2BGR": "BGRA2BGR", "RGBA2BGR": "RGBA2BGR",
            "BGR2BGRA": "BGR2BGRA", "BGR2RGBA": "BGR2RGBA", "BGRA2RGBA": "BGRA2RGBA", "GRAY2BGRA": "GRAY2BGRA", "BGRA2GRAY": "BGRA2GRAY",
            "RGBA2GRAY": "RGBA2GRAY"}


@pytest.mark.parametrize("name", sorted(R.CODES))
def test_restatement_equals_cv2(name):
    cn = R.SOURCE_CHANNELS.get(name, 3)
    rng = np.random.default_rng(sorted(R.CODES).index(name))
    img = rng.integers(0, 256, (256, 256) if cn == 1 else (256, 256, cn), dtype=np.uint8)
    if name in ("HLS2BGR", "HLS2RGB"):
        img[..., 0] %= 181                     # hues cv2 itself produces; the wrap above 180 is stated in DESIGN 4.16
        img[:8, :, 2] = 0                      # and greys
    assert np.array_equal(cv2.cvtColor(img, getattr(cv2, "COLOR_" + CV_NAMES[name])), R.CODES[name](img))
