"""GPU suite for the speckle filter, the surface normals and stereo_planes: vp_filter_speckles_i16 (host images), vp_filter_speckles_dev
on packed device images, on device images with padded strides and in place, and the Python layer, byte for byte against
tests/speckle_restate.py over the cases of tests/speckle_cases.py (the sizes that straddle a tile come from vp_filter_speckles_plan);
the normals bit for bit against tests/normals_restate.py; the chain against the composition of the four restatements."""
import numpy as np
import pytest

import normals_cases as NC
import normals_restate as NR
import speckle_cases as SC
import speckle_restate as R
import stereo_cases as StC
import stereo_restate as StR

pytestmark = pytest.mark.gpu

T = SC.tile()
CASES = SC.cases(T)
FOCAL, BASELINE = 534.48, 0.12


def _dev_call(vp, ctx, img, case, spad=0, dpad=0, in_place=False):
    """vp_filter_speckles_dev; spad / dpad: extra int16 at the end of every row, which must come back untouched"""
    from vision.devmat import DeviceMat
    h, w = img.shape
    sbuf = np.full((h, w + spad), 0x5A5A, np.int16)
    sbuf[:, :w] = img
    ds = DeviceMat.from_host(ctx, sbuf)
    dd = ds if in_place else DeviceMat.from_host(ctx, np.full((h, w + dpad), 12345, np.int16))
    pad = spad if in_place else dpad
    vp.check(vp.lib().vp_filter_speckles_dev(ctx.handle, ds.dev_ptr, 2 * (w + spad), w, h, case["new_val"], case["max_size"], case["max_diff"], dd.dev_ptr, 2 * (w + pad)),
             ctx.handle)
    out = dd.host_copy()
    assert np.all(out[:, w:] == (0x5A5A if in_place else 12345)), "the padding was written"
    if not in_place:
        assert np.array_equal(ds.host_copy(), sbuf), "the source was written"
    return np.ascontiguousarray(out[:, :w])


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_every_entry_form_equals_the_statement(vp, case):
    from vision.devmat import DeviceMat
    from vision.utils import stereo
    img, want = case["image"](), SC.expected(case)
    args = (case["max_size"], case["max_diff"], case["new_val"])
    ctx = vp.default_context()
    diff = lambda got: f"{int((got != want).sum())} pixels differ"
    got = stereo.filter_speckles(img, *args)                                                   # vp_filter_speckles_i16
    assert isinstance(got, np.ndarray) and got.dtype == np.int16 and np.array_equal(got, want), "i16: " + diff(got)
    src = DeviceMat.from_host(ctx, img)
    dev = stereo.filter_speckles(src, *args)
    assert isinstance(dev, DeviceMat) and dev.dtype == np.int16 and dev is not src
    got = dev.host_copy()
    assert np.array_equal(got, want), "dev: " + diff(got)
    assert np.array_equal(src.host_copy(), img), "the Python layer returns a new image"
    got = _dev_call(vp, ctx, img, case, spad=3, dpad=5)                                        # odd paddings: rows of every alignment
    assert np.array_equal(got, want), "padded: " + diff(got)
    got = _dev_call(vp, ctx, img, case, spad=4, dpad=8)                                        # rows that stay 8-byte aligned when w is
    assert np.array_equal(got, want), "padded by quads: " + diff(got)
    got = _dev_call(vp, ctx, img, case, in_place=True)
    assert np.array_equal(got, want), "in place: " + diff(got)
    got = _dev_call(vp, ctx, img, case, spad=1, in_place=True)
    assert np.array_equal(got, want), "in place, padded: " + diff(got)


def test_max_speckle_size_zero_copies_and_the_facade_filters_in_place(vp):
    from vision import cv2_facade as f
    from vision.devmat import DeviceMat
    from vision.utils import stereo
    ctx = vp.default_context()
    img = SC.noise(T + 9, 2 * T + 5, (7, 8, 20), 3, holes=0.03)
    assert np.array_equal(stereo.filter_speckles(img, 0, 0), img)
    assert np.array_equal(_dev_call(vp, ctx, img, dict(new_val=-16, max_size=0, max_diff=0), spad=3, dpad=5), img)
    assert np.array_equal(_dev_call(vp, ctx, img, dict(new_val=-16, max_size=0, max_diff=0), in_place=True), img)
    want = R.filter_speckles(img, -16, 4, 1)
    assert np.array_equal(stereo.filter_speckles(img, 4, 1), want)                             # new_val defaults to invalid_disparity(0)
    work = img.copy()
    got, buf = f.filterSpeckles(work, -16, 4, 1)
    assert got is work and buf is None and np.array_equal(work, want)
    dm = DeviceMat.from_host(ctx, img)
    got, _ = f.filterSpeckles(dm, -16, 4, 1)
    assert got is dm and np.array_equal(dm.host_copy(), want)


def _padded_normals(vp, ctx, depth, f, jump, encode):
    from vision.devmat import DeviceMat
    h, w = depth.shape
    zbuf = np.full((h, w + 3), 777.0, np.float32)
    zbuf[:, :w] = depth
    nbuf = np.full((h, 3 * w + 5), -5.0, np.float32)
    dz, dn = DeviceMat.from_host(ctx, zbuf), DeviceMat.from_host(ctx, nbuf)
    vp.check(vp.lib().vp_normals_from_depth_dev(ctx.handle, dz.dev_ptr, 4 * (w + 3), w, h, f, (w - 1) / 2, (h - 1) / 2, jump, int(encode), dn.dev_ptr, 4 * (3 * w + 5)),
             ctx.handle)
    out = dn.host_copy()
    assert np.all(out[:, 3 * w:] == -5.0), "the result's padding was written"
    return np.ascontiguousarray(out[:, :3 * w]).reshape(h, w, 3)


def test_normals_equal_the_statement_bit_for_bit(vp):
    from vision.devmat import DeviceMat
    from vision.utils import stereo
    ctx = vp.default_context()
    one = stereo.normals_from_depth(NC.wall(3, 3), FOCAL)
    assert NC.same_bits(one, NR.normals_from_depth(NC.wall(3, 3), FOCAL)) and (~np.isnan(one[:, :, 0])).sum() == 1
    assert one[1, 1].tolist() == [0.0, 0.0, -1.0]
    for h, w in ((2, 9), (9, 2)):
        assert np.all(np.isnan(stereo.normals_from_depth(NC.wall(h, w), FOCAL))) and np.all(stereo.normals_from_depth(NC.wall(h, w), FOCAL, encode=True) == 0)
    plane, _ = NC.tilted_plane(45, 67, FOCAL, degrees=35.0)
    for depth in (plane, NC.noisy_depth(45, 67, 1)):
        for jump in (None, 0.08):
            for encode in (False, True):
                want = NR.normals_from_depth(depth, FOCAL, max_jump_m=jump, encode=encode)
                got = stereo.normals_from_depth(depth, FOCAL, max_jump_m=jump, encode=encode)
                assert isinstance(got, np.ndarray) and got.dtype == np.float32 and NC.same_bits(got, want), (jump, encode)
                dev = stereo.normals_from_depth(DeviceMat.from_host(ctx, depth), FOCAL, max_jump_m=jump, encode=encode)
                assert isinstance(dev, DeviceMat) and dev.shape == (45, 67, 3) and NC.same_bits(dev.host_copy(), want), (jump, encode)
                assert NC.same_bits(_padded_normals(vp, ctx, depth, FOCAL, 0.0 if jump is None else jump, encode), want), (jump, encode)
    want = NR.normals_from_depth(plane, FOCAL, cx=30.5, cy=20.25)
    assert NC.same_bits(stereo.normals_from_depth(plane, FOCAL, cx=30.5, cy=20.25), want)


def test_stereo_planes_is_the_composition_of_the_four_statements(vp):
    from vision.devmat import DeviceMat
    from vision.utils import stereo
    ctx = vp.default_context()
    left, right = StC.shifted_pair(40, 160, 7, 7, noise=60)
    p = dict(num_disparities=16, block_size=9, uniqueness_ratio=5)
    disp = StR.disparity(left, right, **{**StR.DEFAULTS, **p})
    clean = R.filter_speckles(disp, -16, 30, 32)
    assert 0 < (clean != disp).sum() < (disp != -16).sum(), "the pair must leave speckles to remove, and something to keep"
    depth = StR.depth_from_disparity(clean, FOCAL, BASELINE)
    normal = NR.normals_from_depth(depth, FOCAL, max_jump_m=0.5, encode=True)
    kw = dict(speckle_window_size=30, speckle_range=2, max_jump_m=0.5, **p)
    got_d, got_n = stereo.stereo_planes(left, right, FOCAL, BASELINE, **kw)
    assert isinstance(got_d, np.ndarray) and isinstance(got_n, np.ndarray)
    assert got_d.tobytes() == depth.tobytes() and NC.same_bits(got_n, normal)
    dev_d, dev_n = stereo.stereo_planes(DeviceMat.from_host(ctx, left), right, FOCAL, BASELINE, **kw)
    assert isinstance(dev_d, DeviceMat) and isinstance(dev_n, DeviceMat) and dev_d.dtype == np.float32 and dev_n.shape == (40, 160, 3)
    assert dev_d.host_copy().tobytes() == depth.tobytes() and NC.same_bits(dev_n.host_copy(), normal)
    raw_d, raw_n = stereo.stereo_planes(left, right, FOCAL, BASELINE, speckle_window_size=0, **p)
    assert raw_d.tobytes() == np.asarray(stereo.stereo_depth(left, right, FOCAL, BASELINE, **p)).tobytes()
    assert raw_d.tobytes() == StR.depth_from_disparity(disp, FOCAL, BASELINE).tobytes()
    assert NC.same_bits(raw_n, NR.normals_from_depth(raw_d, FOCAL, encode=True))
