"""Live comparison of the resize statement (resize_restate.py) with a real OpenCV: what settles the scale precision, the unclamped row
weights and the fx / fy form (resize) wherever cv2 exists.  Skipped where `cv2` is not importable (the build and GPU
images).  CPU-only."""
import numpy as np
import pytest

import frames as F
import resize_restate as RR
from test_resize_statement import CHANGED, UNCHANGED

cv2 = pytest.importorskip("cv2")
if not hasattr(cv2, "connectedComponentsWithStats") or getattr(cv2, "__name__", "") != "cv2" or "vision" in getattr(cv2, "__file__", ""):
    pytest.skip("the cv2 facade of this repo is not a reference", allow_module_level=True)

REAL = [((1080, 1920), (768, 1366)), ((1080, 1920), (720, 1280)), ((1080, 1920), (540, 960)), ((1080, 1920), (360, 640)),
        ((1080, 1920), (512, 512)), ((1080, 1920), (2048, 2048)), ((720, 1280), (400, 640)), ((2160, 3840), (1080, 1920)),
        ((2160, 3840), (768, 1366)), ((360, 640), (1080, 1920)), ((480, 480), (640, 640)), ((2, 3), (5, 7))]


@pytest.mark.parametrize("src,dst", REAL + CHANGED + UNCHANGED)
def test_dsize_equals_cv2(src, dst):
    rng = np.random.default_rng(0)
    for cn in (1, 3, 4):
        img = rng.integers(0, 256, src + (cn,), dtype=np.uint8)
        img = img[:, :, 0].copy() if cn == 1 else img
        assert np.array_equal(cv2.resize(img, dst[::-1], interpolation=cv2.INTER_LINEAR), RR.resize(img, dst[::-1]))


def test_random_pairs_equal_cv2():
    rng = np.random.default_rng(1)
    for i in range(300):
        sw, sh, dw, dh = (int(v) for v in rng.integers(1, 301, 4))
        cn = (1, 3, 4)[i % 3]
        img = rng.integers(0, 256, (sh, sw, cn), dtype=np.uint8)
        img = img[:, :, 0].copy() if cn == 1 else img
        assert np.array_equal(cv2.resize(img, (dw, dh)), RR.resize(img, (dw, dh))), ((sw, sh), (dw, dh), cn)


def test_fx_fy_equals_cv2():
    rng = np.random.default_rng(2)
    img = F.s1_buoy(0, 301, 203)
    for fx, fy in [(0.5, 0.5), (1 / 3, 1 / 3), (0.7, 1.3), (2.0, 2.0), (1.5, 0.25)] + [tuple(rng.uniform(0.1, 3, 2)) for _ in range(20)]:
        for sub in (img, img[:200, :300]):
            sub = np.ascontiguousarray(sub)
            try:
                exp = RR.resize(sub, None, fx, fy)
            except NotImplementedError:
                continue                                 # scale 2 with a partial edge cell: not restated
            assert np.array_equal(cv2.resize(sub, None, fx=fx, fy=fy), exp), (sub.shape, fx, fy)
