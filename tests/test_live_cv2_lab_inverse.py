"""Live comparison of the Lab -> BGR and white-balance statement (lab_inverse_restate.py) with a real OpenCV, wherever `cv2` is
importable (not on the build and GPU images: skipped there).  CPU-only.  It would also show an IPP build of cv2 scaling the last bit
of the box mean differently from the generic filter (open points)."""
import numpy as np
import pytest

import frames as F
import lab_inverse_restate as R

cv2 = pytest.importorskip("cv2")
if not hasattr(cv2, "connectedComponentsWithStats") or getattr(cv2, "__name__", "") != "cv2" or "vision" in getattr(cv2, "__file__", ""):
    pytest.skip("the cv2 facade of this repo is not a reference", allow_module_level=True)


def test_lab2bgr_all_inputs():
    v = np.arange(1 << 24, dtype=np.uint32)
    lab = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    assert np.array_equal(cv2.cvtColor(lab, cv2.COLOR_LAB2BGR), R.lab2bgr(lab))


def _wb(bgr_img):          # utils/color.py:370-378
    lab_img = cv2.cvtColor(bgr_img, cv2.COLOR_BGR2LAB).astype(np.float32)
    lab_l, lab_a, lab_b = cv2.split(lab_img)
    lab_a -= np.mean(lab_a) - 128
    lab_b -= np.mean(lab_b) - 128
    return cv2.cvtColor(cv2.merge((lab_l, lab_a, lab_b)).astype(np.uint8), cv2.COLOR_LAB2BGR)


def _wb_blur(bgr_img, kernel_size):          # utils/color.py:381-392
    kernel_size = 2 * (kernel_size // 2) + 1
    lab_img = cv2.cvtColor(bgr_img, cv2.COLOR_BGR2LAB).astype(np.float32)
    lab_l, lab_a, lab_b = cv2.split(lab_img)
    lab_a -= cv2.blur(lab_a, (kernel_size, kernel_size), 0, borderType=cv2.BORDER_REPLICATE) - 128
    lab_b -= cv2.blur(lab_b, (kernel_size, kernel_size), 0, borderType=cv2.BORDER_REPLICATE) - 128
    return cv2.cvtColor(cv2.merge((lab_l, lab_a, lab_b)).astype(np.uint8), cv2.COLOR_LAB2BGR)


@pytest.mark.parametrize("k", [None, 1, 3, 5, 31, 255])
def test_white_balance(k):
    for bgr in (F.s1_buoy(0, 640, 360), F.s1_buoy(1, 97, 61)):
        lab = cv2.cvtColor(bgr, cv2.COLOR_BGR2LAB)
        if k is None:
            assert np.array_equal(_wb(bgr), R.white_balance_bgr(lab)[0])
        else:
            assert np.array_equal(_wb_blur(bgr, k), R.white_balance_bgr_blur(lab, k))
