"""Opt-in check against a real OpenCV (skipped where cv2 is absent): the statement of tests/remap_restate.py - and with it what the
GPU suite pins - equals cv2.remap, cv2.warpPerspective and cv2.convertMaps byte for byte; the facade's initUndistortRectifyMap is
compared with cv2's maps, and undistort with cv2.undistort within one grey level on the share of pixels the map difference explains.

Measured shares (fill in from a run with cv2 present): not measured yet."""
import numpy as np
import pytest

cv2 = pytest.importorskip("cv2")
if not hasattr(cv2, "getBuildInformation"):
    pytest.skip("cv2 is the stand-in of this package, not OpenCV", allow_module_level=True)

import remap_restate as R  # noqa: E402


def _img(h, w, cn):
    rng = np.random.default_rng(h + 7 * w + cn)
    return rng.integers(0, 256, (h, w) if cn == 1 else (h, w, cn), dtype=np.uint8)


BORDERS = (("constant", cv2.BORDER_CONSTANT), ("replicate", cv2.BORDER_REPLICATE))


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_remap_and_convert_maps_equal_cv2(cn):
    rng = np.random.default_rng(3)
    img = _img(61, 83, cn)
    mx = (rng.integers(-3 * 64, (83 + 3) * 64, (70, 90)) / 64).astype(np.float32)
    my = (rng.integers(-3 * 64, (61 + 3) * 64, (70, 90)) / 64).astype(np.float32)
    val = (9, 80, 170, 250)[:cn]
    for nearest, interp in ((False, cv2.INTER_LINEAR), (True, cv2.INTER_NEAREST)):
        xy, frac = R.convert_maps_restate(mx, my, nearest)
        c1, c2 = cv2.convertMaps(mx, my, cv2.CV_16SC2, nninterpolation=nearest)
        assert np.array_equal(c1, xy) and (nearest or np.array_equal(c2, frac))
        for name, code in BORDERS:
            exp = cv2.remap(img, mx, my, interp, borderMode=code, borderValue=val)
            assert np.array_equal(R.remap_restate(img, mx, my, nearest, name, val), exp)
            assert np.array_equal(cv2.remap(img, np.dstack([mx, my]), None, interp, borderMode=code, borderValue=val), exp)
            if nearest:
                assert np.array_equal(cv2.remap(img, c1, None, interp, borderMode=code, borderValue=val), exp)
            else:
                assert np.array_equal(cv2.remap(img, c1, c2, interp, borderMode=code, borderValue=val), exp)


@pytest.mark.parametrize("size", [(63, 3), (64, 15), (65, 16), (129, 17), (400, 300)])
def test_warp_perspective_equals_cv2(size):
    dw, dh = size
    H = np.array([[1.1, 0.07, -2.3], [-0.04, 0.93, 1.7], [1.0 / (0.6 * dw), 0.031, -0.5]])
    fwd = np.array([[0.9, 0.1, 3.0], [-0.05, 1.1, -2.0], [0.002, -0.001, 1.0]])
    for cn in (1, 3):
        img = _img(41, 53, cn)
        val = (9, 80, 170)[:cn]
        for M, inverse in ((H, True), (fwd, False)):
            for nearest, interp in ((False, cv2.INTER_LINEAR), (True, cv2.INTER_NEAREST)):
                for name, code in BORDERS:
                    flags = interp | (cv2.WARP_INVERSE_MAP if inverse else 0)
                    exp = cv2.warpPerspective(img, M, (dw, dh), flags=flags, borderMode=code, borderValue=val)
                    assert np.array_equal(R.warp_perspective_restate(img, M, (dw, dh), inverse, nearest, name, val), exp), (size, cn, inverse, nearest, name)


def test_undistort_within_one_grey_level_on_the_share_the_maps_explain(capsys):
    from vision import cv2_facade as f
    K = np.array([[812.5, 0.0, 318.25], [0.0, 809.75, 243.5], [0.0, 0.0, 1.0]])
    dist = np.array([-0.31, 0.12, 0.0011, -0.0007, -0.02])
    size = (640, 480)
    mx, my = f.initUndistortRectifyMap(K, dist, None, K, size, f.CV_32FC1)
    cx, cy = cv2.initUndistortRectifyMap(K, dist, None, K, size, cv2.CV_32FC1)
    assert np.abs(mx - cx).max() <= 4 * np.spacing(np.float32(640)) and np.abs(my - cy).max() <= 4 * np.spacing(np.float32(480))
    xy, frac = f.initUndistortRectifyMap(K, dist, None, K, size, f.CV_16SC2)
    c1, c2 = cv2.initUndistortRectifyMap(K, dist, None, K, size, cv2.CV_16SC2)
    differ = (xy != c1).any(axis=2) | (frac != c2)
    share = float(differ.mean())
    yy, xx = np.mgrid[0:480, 0:640]                         # gradients without a wrap, at most 0.4 grey levels per pixel: a 1/32 pixel map
    img = np.dstack([xx * 0.39, yy * 0.5, (xx + yy) * 0.22]).astype(np.uint8)       # step moves a sample by far less than one level
    ours = R.remap_restate(img, xy, frac)
    theirs = cv2.undistort(img, K, dist)
    off = np.abs(ours.astype(int) - theirs.astype(int)).max(axis=2)
    with capsys.disabled():
        print(f"\nundistort: map entries that differ from cv2's: {share:.6f}; pixels that differ: {float((off > 0).mean()):.6f}; largest difference {int(off.max())}")
    assert (off > 0).mean() <= share, "more pixels differ than map entries do"
    assert off.max() <= 1, "undistort differs from cv2 by more than one grey level"
