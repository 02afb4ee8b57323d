"""GPU suite for semi-global matching: vp_stereo_sgm_u8 (host images), vp_stereo_sgm_dev on packed device images and on device images
with padded strides, and the Python layer, all byte for byte against the expectation of every case of tests/sgm_cases.py (the numpy
statement; vp_stereo_sgm_host for the mid-size case) - the sizes that straddle the kernels' geometry come from vp_stereo_sgm_plan."""
import numpy as np
import pytest

import sgm_cases as SC
import sgm_restate as G
import stereo_restate as R
from stereo_cases import shifted_pair, two_plane_pair

pytestmark = pytest.mark.gpu

CASES = SC.cases(SC.lib_plan)
FOCAL, BASELINE = 534.48, 0.12


def _padded_dev(vp, ctx, left, right, params, pads=(5, 3, 4)):
    """vp_stereo_sgm_dev on images whose rows are longer than the image, the result's too; the padding must come back untouched"""
    from vision.devmat import DeviceMat
    h, w = left.shape
    lp, rp, dp = pads
    lbuf, rbuf = np.full((h, w + lp), 0xA5, np.uint8), np.full((h, w + rp), 0x5A, np.uint8)
    lbuf[:, :w], rbuf[:, :w] = left, right
    dbuf = np.full((h, w + dp), 12345, np.int16)
    dl, dr, dd = DeviceMat.from_host(ctx, lbuf), DeviceMat.from_host(ctx, rbuf), DeviceMat.from_host(ctx, dbuf)
    vp.check(vp.lib().vp_stereo_sgm_dev(ctx.handle, dl.dev_ptr, w + lp, dr.dev_ptr, w + rp, w, h, *SC.ordered(params), dd.dev_ptr, 2 * (w + dp)), ctx.handle)
    out = dd.host_copy()
    assert np.all(out[:, w:] == 12345), "the result's padding was written"
    return np.ascontiguousarray(out[:, :w])


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_every_entry_form_equals_the_expectation(vp, case):
    from vision.devmat import DeviceMat
    from vision.utils import stereo
    left, right = case["pair"]()
    want, p = SC.expected(case), case["params"]
    ctx = vp.default_context()
    got = stereo.disparity_sgm(left, right, **p)                               # host images in, host image out
    assert isinstance(got, np.ndarray) and got.dtype == np.int16 and np.array_equal(got, want), f"u8: {int((got != want).sum())} pixels differ"
    dev = stereo.disparity_sgm(DeviceMat.from_host(ctx, left), DeviceMat.from_host(ctx, right), **p)
    assert isinstance(dev, DeviceMat) and dev.dtype == np.int16
    got = dev.host_copy()
    assert np.array_equal(got, want), f"dev: {int((got != want).sum())} pixels differ"
    if case["oracle"] == "statement":                                          # the mid-size case is excepted from the padded form
        got = _padded_dev(vp, ctx, left, right, p)
        assert np.array_equal(got, want), f"padded: {int((got != want).sum())} pixels differ"


def test_calls_of_different_sizes_carry_nothing_over(vp):
    """the grow-only workspace and the S volume: a larger call with more disparities between two runs of a smaller one"""
    from vision.utils import stereo
    ids = {c["id"]: c for c in CASES}
    first, second = ids["nd_32_p8"], ids["nd_128_p4"]
    for case in (first, second, first):
        got = stereo.disparity_sgm(*case["pair"](), **case["params"])
        assert np.array_equal(got, SC.expected(case)), case["id"]


def test_depth_chain_stays_on_the_device(vp):
    from vision.devmat import DeviceMat
    from vision.utils import stereo
    left, right = two_plane_pair(40, 160, 7)
    p = dict(num_disparities=16, block_size=5, p1=8, p2=32)
    want = R.depth_from_disparity(G.disparity(left, right, **p), FOCAL, BASELINE)
    assert np.count_nonzero(want) > 1000
    ctx = vp.default_context()
    chained = stereo.stereo_depth_sgm(DeviceMat.from_host(ctx, left), DeviceMat.from_host(ctx, right), FOCAL, BASELINE, **p)
    assert isinstance(chained, DeviceMat) and chained.dtype == np.float32 and chained.host_copy().tobytes() == want.tobytes()
    got = stereo.stereo_depth_sgm(left, right, FOCAL, BASELINE, **p)
    assert isinstance(got, np.ndarray) and got.tobytes() == want.tobytes()


def test_planes_chain_is_the_four_steps_composed(vp):
    from vision.devmat import DeviceMat
    from vision.utils import stereo
    left, right = shifted_pair(40, 160, 6, 7, noise=30)
    p = dict(num_disparities=16, block_size=5, min_disparity=1)
    disp = stereo.disparity_sgm(left, right, **p)
    disp = stereo.filter_speckles(disp, 30, 16 * 2, stereo.invalid_disparity(1))
    depth = stereo.depth_from_disparity(disp, FOCAL, BASELINE)
    normal = stereo.normals_from_depth(depth, FOCAL, max_jump_m=0.5, encode=True)
    assert np.count_nonzero(depth) > 500 and np.count_nonzero(normal) > 500
    got = stereo.stereo_planes_sgm(left, right, FOCAL, BASELINE, speckle_window_size=30, speckle_range=2, max_jump_m=0.5, **p)
    assert all(isinstance(a, np.ndarray) for a in got) and got[0].tobytes() == depth.tobytes() and got[1].tobytes() == normal.tobytes()
    ctx = vp.default_context()
    dev = stereo.stereo_planes_sgm(DeviceMat.from_host(ctx, left), DeviceMat.from_host(ctx, right), FOCAL, BASELINE, speckle_window_size=30, speckle_range=2,
                                   max_jump_m=0.5, **p)
    assert all(isinstance(a, DeviceMat) for a in dev) and dev[0].host_copy().tobytes() == depth.tobytes() and dev[1].host_copy().tobytes() == normal.tobytes()


def test_colour_pairs_go_through_bgr_to_gray(vp):
    from vision.utils import color, stereo
    left, right = shifted_pair(36, 110, 10, 8)
    rng = np.random.default_rng(5)
    bl = np.clip(left[:, :, None].astype(np.int32) + rng.integers(-20, 21, (36, 110, 3)), 0, 255).astype(np.uint8)
    br = np.clip(right[:, :, None].astype(np.int32) + rng.integers(-20, 21, (36, 110, 3)), 0, 255).astype(np.uint8)
    p = dict(num_disparities=32, block_size=5)
    want = G.disparity(np.asarray(color.bgr_to_gray(bl)[0]), np.asarray(color.bgr_to_gray(br)[0]), **p)
    assert np.any(want != -16)
    assert np.array_equal(stereo.disparity_sgm(bl, br, **p), want)
