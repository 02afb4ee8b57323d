"""GPU suite for stereo block matching: vp_stereo_bm_u8 (host images), vp_stereo_bm_dev on packed device images and on device images
with padded strides, and the Python layer, all byte for byte against tests/stereo_restate.py over the cases of tests/stereo_cases.py -
the sizes that straddle the matcher's strip and band come from vp_stereo_bm_plan."""
import numpy as np
import pytest

import stereo_cases as SC
import stereo_restate as R

pytestmark = pytest.mark.gpu

CASES = SC.cases(SC.lib_plan)
FOCAL, BASELINE = 534.48, 0.12


def _padded_dev(vp, ctx, left, right, params, pads=(5, 3, 4)):
    """vp_stereo_bm_dev on images whose rows are longer than the image, the result's too; the padding must come back untouched"""
    from vision.devmat import DeviceMat
    h, w = left.shape
    lp, rp, dp = pads
    lbuf, rbuf = np.full((h, w + lp), 0xA5, np.uint8), np.full((h, w + rp), 0x5A, np.uint8)
    lbuf[:, :w], rbuf[:, :w] = left, right
    dbuf = np.full((h, w + dp), 12345, np.int16)
    dl, dr, dd = DeviceMat.from_host(ctx, lbuf), DeviceMat.from_host(ctx, rbuf), DeviceMat.from_host(ctx, dbuf)
    p = params
    vp.check(vp.lib().vp_stereo_bm_dev(ctx.handle, dl.dev_ptr, w + lp, dr.dev_ptr, w + rp, w, h, p["num_disparities"], p["block_size"], p["min_disparity"],
                                       p["pre_filter_cap"], p["texture_threshold"], p["uniqueness_ratio"], dd.dev_ptr, 2 * (w + dp)), ctx.handle)
    out = dd.host_copy()
    assert np.all(out[:, w:] == 12345), "the result's padding was written"
    return np.ascontiguousarray(out[:, :w])


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_both_entry_forms_equal_the_statement(vp, case):
    from vision.devmat import DeviceMat
    from vision.utils import stereo
    left, right = case["pair"]()
    want, p = SC.expected(case), case["params"]
    ctx = vp.default_context()
    got = stereo.disparity(left, right, **p)                                   # host images in, host image out
    assert isinstance(got, np.ndarray) and got.dtype == np.int16 and np.array_equal(got, want), f"u8: {int((got != want).sum())} pixels differ"
    dev = stereo.disparity(DeviceMat.from_host(ctx, left), DeviceMat.from_host(ctx, right), **p)
    assert isinstance(dev, DeviceMat) and dev.dtype == np.int16
    got = dev.host_copy()
    assert np.array_equal(got, want), f"dev: {int((got != want).sum())} pixels differ"
    if case["id"] != "hd720":
        got = _padded_dev(vp, ctx, left, right, p)
        assert np.array_equal(got, want), f"padded: {int((got != want).sum())} pixels differ"


def test_cases_cover_what_they_claim():
    ids = {c["id"]: c for c in CASES}
    one = SC.expected(ids["tiny_5x20"])
    assert (one != -16).sum() == 1 and one[2, 17] != -16                       # exactly one candidate pixel, and it is answered
    assert np.all(SC.expected(ids["tiny_5x19"]) == -16) and np.all(SC.expected(ids["tiny_4x40"]) == -16)
    assert SC.expected(ids["cap_63"]).max() > 0
    assert np.all(SC.expected(ids["texture_above"]) == -16) and np.any(SC.expected(ids["texture_at"]) != -16)
    assert np.any(SC.expected(ids["uniq_100"]) != SC.expected(ids["uniq_0"]))
    band = SC.lib_plan(60, 200, 16, 9, 0)["band_rows"]
    assert SC.lib_plan(60, 9 + band, 16, 9, 0)["grid"][1] == 2 and SC.lib_plan(60, 8 + band, 16, 9, 0)["grid"][1] == 1
    for n in (16, 256):
        strip = SC.lib_plan(400, 40, n, 5, 0)["strip_cols"]
        assert [SC.lib_plan(cw + 4 + n - 1, 7, n, 5, 0)["grid"][0] for cw in (strip - 1, strip, strip + 1, 2 * strip)] == [1, 1, 2, 2]


def test_depth_forms_and_the_chain_stay_on_the_device(vp):
    from vision.devmat import DeviceMat
    from vision.utils import stereo
    left, right = SC.two_plane_pair(40, 160, 7)
    p = dict(num_disparities=16, block_size=9)
    disp = R.disparity(left, right, **p)
    want = R.depth_from_disparity(disp, FOCAL, BASELINE)
    assert np.count_nonzero(want) > 1000
    got = stereo.depth_from_disparity(disp, FOCAL, BASELINE)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.tobytes() == want.tobytes()
    ctx = vp.default_context()
    dev = stereo.depth_from_disparity(DeviceMat.from_host(ctx, disp), FOCAL, BASELINE)
    assert isinstance(dev, DeviceMat) and dev.host_copy().tobytes() == want.tobytes()
    chained = stereo.stereo_depth(DeviceMat.from_host(ctx, left), DeviceMat.from_host(ctx, right), FOCAL, BASELINE, **p)
    assert isinstance(chained, DeviceMat) and chained.dtype == np.float32 and chained.host_copy().tobytes() == want.tobytes()
    assert stereo.stereo_depth(left, right, FOCAL, BASELINE, **p).tobytes() == want.tobytes()
    # every int16 value through the quotient, on padded device rows
    every = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16).reshape(256, 256)
    assert stereo.depth_from_disparity(every, FOCAL, BASELINE).tobytes() == R.depth_from_disparity(every, FOCAL, BASELINE).tobytes()


def test_colour_pairs_and_the_facade(vp):
    from vision import cv2_facade as f
    from vision.utils import color, stereo
    left, right = SC.shifted_pair(36, 150, 10, 8)
    rng = np.random.default_rng(5)
    bl = np.clip(left[:, :, None].astype(np.int32) + rng.integers(-20, 21, (36, 150, 3)), 0, 255).astype(np.uint8)
    br = np.clip(right[:, :, None].astype(np.int32) + rng.integers(-20, 21, (36, 150, 3)), 0, 255).astype(np.uint8)
    p = dict(num_disparities=32, block_size=7)
    want = R.disparity(np.asarray(color.bgr_to_gray(bl)[0]), np.asarray(color.bgr_to_gray(br)[0]), **p)
    assert np.array_equal(stereo.disparity(bl, br, **p), want)
    bm = f.StereoBM_create(32, 7)
    got = bm.compute(left, right)
    assert got.dtype == np.int16 and np.array_equal(got, R.disparity(left, right, **dict(R.DEFAULTS, **p)))
    bm.setUniquenessRatio(0)
    bm.setMinDisparity(2)
    assert np.array_equal(bm.compute(left, right), R.disparity(left, right, **dict(R.DEFAULTS, **p, uniqueness_ratio=0, min_disparity=2)))
