"""GPU suite for cv2.remap / convertMaps / warpPerspective (vp_remap_*, vp_convert_maps_dev, vp_warp_perspective_*, vision.cv2_facade,
vision.utils.transform).

Every comparison is byte for byte against tests/remap_restate.py, never against the library under test.  The kernels' tile is RM_TW
destination pixels x RM_TH rows with RM_PPT pixels per lane (read here from csrc/vp_remap_plan.h): the shapes are that tile exactly,
one pixel more and less in each direction, the smallest images and ragged multi-channel ones.  Rows that are whole groups of RM_PPT
pixels take the vector loads and stores, the others the scalar ones; both are among the shapes.  No test provokes a fault: every
invalid call is one the host check turns away before a launch."""
import functools
import os
import re

import numpy as np
import pytest

import remap_restate as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PLAN = open(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc", "vp_remap_plan.h")).read()
TW = int(re.search(r"#define RM_TW (\d+)", _PLAN).group(1))
TH = int(re.search(r"#define RM_TH (\d+)", _PLAN).group(1))

TINY = [(1, 1, 1), (1, 9, 1), (9, 1, 1), (2, 2, 1)]                                                       # map (h, w), cn
TILE = [(TH, TW, 1), (TH + 1, TW, 1), (TH - 1, TW, 1), (TH, TW + 1, 1), (TH, TW - 1, 1)]
RAGGED = [(67, 35, 1), (67, 35, 3), (67, 35, 4), (301, 203, 3), (36, 68, 2), (36, 68, 3), (36, 68, 4)]
BORDERS = [("constant", 0), ("replicate", 1)]
VALUE = (201, 17, 99, 250)
SRC_H, SRC_W = 41, 53                                                                                     # differs from every map size


@functools.lru_cache(maxsize=None)
def _image(h, w, cn):
    rng = np.random.default_rng(h * 1009 + w * 31 + cn * 7)
    a = rng.integers(0, 256, (h, w) if cn == 1 else (h, w, cn), dtype=np.uint8)
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def _maps(kind, h, w, sh, sw):
    """float32 (mapx, mapy) of shape (h, w) into a source of sh x sw"""
    y, x = np.mgrid[0:h, 0:w]
    x, y = x.astype(np.float32), y.astype(np.float32)
    rng = np.random.default_rng(h * 7919 + w * 13 + sh)
    if kind == "identity":
        mx, my = x, y
    elif kind == "outside":
        mx, my = x + np.float32(sw + 5), y - np.float32(sh + 5)
    elif kind == "random":                                   # a 1/64 grid: half of the values are cvRound ties
        mx = (rng.integers(-3 * 64, (sw + 3) * 64 + 1, (h, w)) / 64).astype(np.float32)
        my = (rng.integers(-3 * 64, (sh + 3) * 64 + 1, (h, w)) / 64).astype(np.float32)
    elif kind == "barrel":
        from vision import cv2_facade as f
        Kc = np.array([[0.9 * sw, 0.0, sw / 2 - 0.3], [0.0, 0.9 * sw, sh / 2 + 0.2], [0.0, 0.0, 1.0]])
        Kn = np.array([[0.9 * sw * w / sw, 0.0, w / 2], [0.0, 0.9 * sw * h / sh, h / 2], [0.0, 0.0, 1.0]])
        mx, my = f.initUndistortRectifyMap(Kc, [-0.35, 0.15, 0.002, -0.001, -0.03], None, Kn, (w, h), f.CV_32FC1)
    else:
        assert kind == "saturating"
        big = np.float32([32767.0, 32768.0, 40000.0, 6.0e7, -32768.0, -32769.0, -6.0e7, 32767.96875, -0.5, 0.5, sw - 0.5, -1.0])
        mx = big[rng.integers(0, len(big), (h, w))]
        my = big[rng.integers(0, len(big), (h, w))]
    mx, my = np.ascontiguousarray(mx, np.float32), np.ascontiguousarray(my, np.float32)
    mx.flags.writeable = my.flags.writeable = False
    return mx, my


MAP_KINDS = ["identity", "outside", "random", "barrel", "saturating"]


@functools.lru_cache(maxsize=None)
def _expect(kind, h, w, cn, nearest, border, sh=SRC_H, sw=SRC_W):
    mx, my = _maps(kind, h, w, sh, sw)
    out = R.remap_restate(_image(sh, sw, cn), mx, my, nearest, border, VALUE[:cn])
    out.flags.writeable = False
    return out


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _dev(ctx, arr):
    from vision.devmat import DeviceMat
    return DeviceMat.from_host(ctx, arr)


def _bv(vp):
    return np.array(VALUE, np.uint8)


def _run_all_forms(vp, kind, h, w, cn, nearest, border, code):
    """host entry, float device entry (planar and interleaved), convert + fixed device entry: all against the statement"""
    from vision.devmat import DeviceMat
    ctx, L = vp.default_context(), vp.lib()
    img = _image(SRC_H, SRC_W, cn)
    mx, my = _maps(kind, h, w, SRC_H, SRC_W)
    exp = _expect(kind, h, w, cn, nearest, border)
    interp = vp.INTER_NEAREST if nearest else vp.INTER_LINEAR
    bv = _bv(vp)
    tag = (kind, h, w, cn, nearest, border)
    out = np.empty_like(exp)
    vp.check(L.vp_remap_u8(ctx.handle, vp.ptr(np.ascontiguousarray(img)), SRC_W, SRC_H, cn, vp.ptr(mx), vp.ptr(my), w, h, interp, code, vp.ptr(bv), vp.ptr(out)), ctx.handle)
    assert _same(out, exp), tag + ("host entry",)
    src, dx, dy, dxy = _dev(ctx, img), _dev(ctx, mx), _dev(ctx, my), _dev(ctx, np.dstack([mx, my]))
    for name, a, b in (("planar", dx, dy), ("interleaved", dxy, None)):
        dst = DeviceMat(ctx, exp.shape)
        vp.check(L.vp_remap_f32_dev(ctx.handle, src.dev_ptr, SRC_W * cn, SRC_W, SRC_H, cn, a.dev_ptr, None if b is None else b.dev_ptr, w, h, interp, code, vp.ptr(bv),
                                    dst.dev_ptr), ctx.handle)
        assert _same(np.asarray(dst), exp), tag + (name,)
    xy = DeviceMat(ctx, (h, w, 2), np.int16)
    frac = None if nearest else DeviceMat(ctx, (h, w), np.uint16)
    vp.check(L.vp_convert_maps_dev(ctx.handle, dx.dev_ptr, dy.dev_ptr, w, h, int(nearest), xy.dev_ptr, None if frac is None else frac.dev_ptr), ctx.handle)
    exy, efrac = R.convert_maps_restate(mx, my, nearest)
    assert _same(np.asarray(xy), exy), tag + ("convertMaps xy",)
    if not nearest:
        assert _same(np.asarray(frac), efrac), tag + ("convertMaps fractions",)
    dst = DeviceMat(ctx, exp.shape)
    vp.check(L.vp_remap_fixed_dev(ctx.handle, src.dev_ptr, SRC_W * cn, SRC_W, SRC_H, cn, xy.dev_ptr, None if frac is None else frac.dev_ptr, w, h, interp, code,
                                  vp.ptr(bv), dst.dev_ptr), ctx.handle)
    assert _same(np.asarray(dst), exp), tag + ("fixed",)


@pytest.mark.parametrize("shape", TINY + TILE + RAGGED)
def test_every_entry_at_every_shape_equals_the_statement(vp, shape):
    h, w, cn = shape
    for nearest in (False, True):
        for border, code in BORDERS:
            _run_all_forms(vp, "random", h, w, cn, nearest, border, code)


@pytest.mark.parametrize("kind", MAP_KINDS)
def test_every_map_at_both_interpolations_and_borders(vp, kind):
    for h, w, cn in ((67, 35, 3), (36, 68, 1)):
        for nearest in (False, True):
            for border, code in BORDERS:
                _run_all_forms(vp, kind, h, w, cn, nearest, border, code)


def test_a_source_read_through_a_stride_and_unaligned_maps(vp):
    """the source is a window of a wider image; the maps start 4 bytes into their allocations, so rows of whole groups take the scalar path"""
    from vision.devmat import DeviceMat
    ctx, L = vp.default_context(), vp.lib()
    for cn in (1, 3):
        wide = _image(SRC_H, SRC_W + 11, cn)
        win = np.ascontiguousarray(wide[:, 3:3 + SRC_W])
        h, w = 36, 68
        mx, my = _maps("random", h, w, SRC_H, SRC_W)
        dwide = _dev(ctx, wide)
        bv = _bv(vp)
        pad = lambda a: np.concatenate([np.zeros(1, np.float32), a.ravel()])
        px, py, ax, ay = _dev(ctx, pad(mx)), _dev(ctx, pad(my)), _dev(ctx, mx), _dev(ctx, my)
        for nearest in (False, True):
            exp = R.remap_restate(win, mx, my, nearest, "constant", VALUE[:cn])
            for a, b in ((ax.dev_ptr, ay.dev_ptr), (px.dev_ptr + 4, py.dev_ptr + 4)):
                dst = DeviceMat(ctx, exp.shape)
                vp.check(L.vp_remap_f32_dev(ctx.handle, dwide.dev_ptr + 3 * cn, (SRC_W + 11) * cn, SRC_W, SRC_H, cn, a, b, w, h, 0 if nearest else 1, 0, vp.ptr(bv),
                                            dst.dev_ptr), ctx.handle)
                assert _same(np.asarray(dst), exp), (cn, nearest)


def test_misaligned_planes_take_the_scalar_path_in_every_launcher(vp):
    """rows are whole groups of RM_PPT pixels, so only the pointers decide: the fixed-form planes (written there by vp_convert_maps_dev)
    and the destinations of vp_remap_fixed_dev and vp_warp_perspective_dev start 2 and 1 bytes into their allocations"""
    from vision.devmat import DeviceMat
    ctx, L = vp.default_context(), vp.lib()
    h, w = 36, 68
    mx, my = _maps("random", h, w, SRC_H, SRC_W)
    dx, dy = _dev(ctx, mx), _dev(ctx, my)
    bv = _bv(vp)
    fwd = np.array([[0.9, 0.1, 3.0], [-0.05, 1.1, -2.0], [0.002, -0.001, 1.0]])
    for cn in (1, 3, 4):
        img = _image(SRC_H, SRC_W, cn)
        src = _dev(ctx, img)
        shape = (h, w) if cn == 1 else (h, w, cn)
        for nearest in (False, True):
            exp = _expect("random", h, w, cn, nearest, "constant")
            exy, efrac = R.convert_maps_restate(mx, my, nearest)
            for oxy, ofr, odst in ((2, 2, 0), (0, 2, 0), (0, 0, 1), (2, 0, 1)):
                xy = _dev(ctx, np.full(h * w * 2 + 8, -5, np.int16))
                frac = _dev(ctx, np.full(h * w + 8, 7, np.uint16))
                dst = _dev(ctx, np.full(h * w * cn + 16, 55, np.uint8))
                fp = None if nearest else frac.dev_ptr + ofr
                vp.check(L.vp_convert_maps_dev(ctx.handle, dx.dev_ptr, dy.dev_ptr, w, h, int(nearest), xy.dev_ptr + oxy, fp), ctx.handle)
                vp.check(L.vp_remap_fixed_dev(ctx.handle, src.dev_ptr, SRC_W * cn, SRC_W, SRC_H, cn, xy.dev_ptr + oxy, fp, w, h, 0 if nearest else 1, 0, vp.ptr(bv),
                                              dst.dev_ptr + odst), ctx.handle)
                gxy, gfr, got = xy.host_copy(), frac.host_copy(), dst.host_copy()
                tag = (cn, nearest, oxy, ofr, odst)
                assert _same(gxy[oxy // 2:oxy // 2 + h * w * 2].reshape(h, w, 2), exy) and (gxy[:oxy // 2] == -5).all() and (gxy[oxy // 2 + h * w * 2:] == -5).all(), tag
                if nearest:
                    assert (gfr == 7).all(), tag
                else:
                    assert _same(gfr[ofr // 2:ofr // 2 + h * w].reshape(h, w), efrac) and (gfr[:ofr // 2] == 7).all() and (gfr[ofr // 2 + h * w:] == 7).all(), tag
                assert _same(got[odst:odst + h * w * cn].reshape(shape), exp) and (got[:odst] == 55).all() and (got[odst + h * w * cn:] == 55).all(), tag
            for odst in (1, 4):
                dst = _dev(ctx, np.full(h * w * cn + 16, 55, np.uint8))
                M = np.ascontiguousarray(fwd)
                vp.check(L.vp_warp_perspective_dev(ctx.handle, src.dev_ptr, SRC_W * cn, SRC_W, SRC_H, cn, vp.ptr(M), 0 if nearest else 1, 0, vp.ptr(bv),
                                                   dst.dev_ptr + odst, w, h), ctx.handle)
                got = dst.host_copy()
                want = R.warp_perspective_restate(img, fwd, (w, h), False, nearest, "constant", VALUE[:cn])
                assert _same(got[odst:odst + h * w * cn].reshape(shape), want) and (got[:odst] == 55).all() and (got[odst + h * w * cn:] == 55).all(), (cn, nearest, odst)


def test_facade_and_transform_with_device_and_numpy_operands(vp):
    from vision import cv2_facade as f
    from vision.devmat import DeviceMat
    from vision.utils import transform
    ctx = vp.default_context()
    h, w, cn = 67, 35, 3
    img = _image(SRC_H, SRC_W, cn)
    mx, my = _maps("random", h, w, SRC_H, SRC_W)
    for nearest, interp in ((False, f.INTER_LINEAR), (True, f.INTER_NEAREST)):
        for border, code in BORDERS:
            exp = _expect("random", h, w, cn, nearest, border)
            xy, frac = R.convert_maps_restate(mx, my, nearest)
            forms = [(mx, my), (np.dstack([mx, my]), None), (xy, frac)]
            for m1, m2 in forms:
                host = f.remap(img, m1, m2, interp, None, code, VALUE)
                assert type(host) is np.ndarray and _same(host, exp), (nearest, border, "numpy")
                src = _dev(ctx, img)
                out = f.remap(src, _dev(ctx, m1), None if m2 is None else _dev(ctx, m2), interp, None, code, VALUE)
                assert isinstance(out, DeviceMat) and src._host is None and out._host is None, "a host copy was made"
                assert _same(np.asarray(out), exp), (nearest, border, "device")
                assert _same(np.asarray(f.remap(_dev(ctx, img), m1, m2, interp, borderMode=code, borderValue=VALUE)), exp), "device image, numpy maps"
            assert _same(transform.remap(img, mx, my, nearest, code, VALUE), exp)
            c1, c2 = f.convertMaps(mx, my, f.CV_16SC2, nearest)
            assert _same(c1, xy) and (c2.size == 0 if nearest else _same(c2, frac))
            d1, d2 = f.convertMaps(_dev(ctx, np.dstack([mx, my])), None, f.CV_16SC2, nearest)
            assert isinstance(d1, DeviceMat) and _same(np.asarray(d1), xy) and (d2.size == 0 if nearest else _same(np.asarray(d2), frac))
    dst = np.zeros((h, w, cn), np.uint8)
    assert f.remap(img, mx, my, f.INTER_LINEAR, dst) is dst and _same(dst, R.remap_restate(img, mx, my))


def test_remap_table_applied_twice_equals_remap(vp):
    from vision.devmat import DeviceMat
    from vision.utils import transform
    ctx = vp.default_context()
    for h, w, cn in ((67, 35, 3), (36, 68, 1)):
        img = _image(SRC_H, SRC_W, cn)
        mx, my = _maps("barrel", h, w, SRC_H, SRC_W)
        for nearest in (False, True):
            table = transform.RemapTable(mx, my, nearest)
            assert table.shape == (h, w) and (table.frac is None) == nearest
            src = _dev(ctx, img)
            first = table.apply(src, 1)
            second = table.apply(src, 1)
            assert isinstance(first, DeviceMat) and src._host is None
            exp = _expect("barrel", h, w, cn, nearest, "replicate")
            assert _same(np.asarray(first), exp) and _same(np.asarray(second), exp)
            assert _same(np.asarray(transform.remap(src, mx, my, nearest, 1)), exp)
            assert _same(table.apply(img, 0, VALUE), _expect("barrel", h, w, cn, nearest, "constant"))


def test_undistort_and_undistorter(vp):
    from vision import cv2_facade as f
    from vision.utils import transform
    ctx = vp.default_context()
    img = _image(SRC_H, SRC_W, 3)
    Kc = np.array([[48.0, 0.0, 26.2], [0.0, 47.5, 20.7], [0.0, 0.0, 1.0]])
    dist = [-0.3, 0.1, 0.001, -0.002, 0.0]
    xy, frac = f.initUndistortRectifyMap(Kc, dist, None, Kc, (SRC_W, SRC_H), f.CV_16SC2)
    exp = R.remap_restate(img, xy, frac)
    assert _same(f.undistort(img, Kc, dist), exp)
    assert _same(np.asarray(f.undistort(_dev(ctx, img), Kc, dist)), exp)
    mx, my = f.initUndistortRectifyMap(Kc, dist, None, Kc, (SRC_W, SRC_H), f.CV_32FC1)
    table = transform.undistorter(Kc, dist, (SRC_W, SRC_H))
    assert _same(np.asarray(table.apply(_dev(ctx, img))), R.remap_restate(img, mx, my))


# a true projective matrix (destination -> source) whose denominator crosses zero inside the first rows of every size below
def _projective(dw, dh):
    return np.array([[1.1, 0.07, -2.3], [-0.04, 0.93, 1.7], [1.0 / (0.6 * dw), 0.031, -0.5]])


WP_SIZES = [(63, 3), (64, 15), (65, 16), (129, 17), (64, 3), (129, 16)]


@pytest.mark.parametrize("size", WP_SIZES)
def test_warp_perspective_every_block_width_both_flags(vp, size):
    from vision import cv2_facade as f
    from vision.devmat import DeviceMat
    ctx, L = vp.default_context(), vp.lib()
    dw, dh = size
    H = _projective(dw, dh)
    m = H.ravel()
    w = m[6] * np.arange(dw)[None, :] + m[7] * np.arange(dh)[:, None] + m[8]
    assert (w[0] < 0).any() and (w[0] > 0).any(), "the denominator must change sign inside a row"
    fwd = np.array([[0.9, 0.1, 3.0], [-0.05, 1.1, -2.0], [0.002, -0.001, 1.0]])
    for cn in (1, 3, 4):
        img = _image(SRC_H, SRC_W, cn)
        src = _dev(ctx, img)
        for M, inverse in ((H, True), (fwd, False)):
            for nearest in (False, True):
                for border, code in BORDERS:
                    exp = R.warp_perspective_restate(img, M, (dw, dh), inverse, nearest, border, VALUE[:cn])
                    flags = (f.WARP_INVERSE_MAP if inverse else 0) | (f.INTER_NEAREST if nearest else f.INTER_LINEAR)
                    tag = (size, cn, inverse, nearest, border)
                    host = f.warpPerspective(img, M, (dw, dh), None, flags, code, VALUE)
                    assert type(host) is np.ndarray and _same(host, exp), tag + ("host entry",)
                    out = f.warpPerspective(src, M, (dw, dh), None, flags, code, VALUE)
                    assert isinstance(out, DeviceMat) and src._host is None and _same(np.asarray(out), exp), tag + ("device entry",)
    # the device entry through a stride
    wide = _image(SRC_H, SRC_W + 11, 3)
    win = np.ascontiguousarray(wide[:, 3:3 + SRC_W])
    dst = DeviceMat(ctx, (dh, dw, 3))
    M = np.ascontiguousarray(fwd)
    vp.check(L.vp_warp_perspective_dev(ctx.handle, _dev(ctx, wide).dev_ptr + 9, (SRC_W + 11) * 3, SRC_W, SRC_H, 3, vp.ptr(M), 1, 0, None, dst.dev_ptr, dw, dh), ctx.handle)
    assert _same(np.asarray(dst), R.warp_perspective_restate(win, fwd, (dw, dh)))


def test_warp_perspective_transform_name_and_exact_affine_case(vp, oracle):
    from vision.utils import transform
    img = _image(SRC_H, SRC_W, 3)
    M = np.array([[0.5, 0.0, 3.0], [0.0, 2.0, -4.0], [0.0, 0.0, 1.0]])
    out = transform.warp_perspective(img, M, 50, 40)
    assert _same(out, R.warp_perspective_restate(img, M, (50, 40)))
    assert _same(out, oracle.warp_affine(img, M[:2], (50, 40)))


def test_argument_errors_return_invalid_and_launch_nothing(vp):
    from vision.devmat import DeviceMat
    ctx, L = vp.default_context(), vp.lib()
    h, w, cn = 8, 12, 1
    img = _image(SRC_H, SRC_W, cn)
    mx, my = _maps("identity", h, w, SRC_H, SRC_W)
    src, dx, dy = _dev(ctx, img), _dev(ctx, mx), _dev(ctx, my)
    xy, frac = DeviceMat(ctx, (h, w, 2), np.int16), DeviceMat(ctx, (h, w), np.uint16)
    vp.check(L.vp_convert_maps_dev(ctx.handle, dx.dev_ptr, dy.dev_ptr, w, h, 0, xy.dev_ptr, frac.dev_ptr), ctx.handle)
    dst = _dev(ctx, np.full((h, w), 77, np.uint8))
    S, X, Y, Q, F, D = src.dev_ptr, dx.dev_ptr, dy.dev_ptr, xy.dev_ptr, frac.dev_ptr, dst.dev_ptr
    sw, sh = SRC_W, SRC_H
    M = np.eye(3)
    nan = np.full((3, 3), np.nan)
    hs, hd = np.ascontiguousarray(img), np.full((h, w), 77, np.uint8)
    bad = [
        lambda: L.vp_remap_f32_dev(ctx.handle, None, sw, sw, sh, cn, X, Y, w, h, 1, 0, None, D),
        lambda: L.vp_remap_f32_dev(ctx.handle, S, sw, sw, sh, cn, None, Y, w, h, 1, 0, None, D),
        lambda: L.vp_remap_f32_dev(ctx.handle, S, sw, sw, sh, cn, X, Y, w, h, 1, 0, None, None),
        lambda: L.vp_remap_f32_dev(ctx.handle, S, sw, sw, sh, 0, X, Y, w, h, 1, 0, None, D),
        lambda: L.vp_remap_f32_dev(ctx.handle, S, sw, sw, sh, 5, X, Y, w, h, 1, 0, None, D),
        lambda: L.vp_remap_f32_dev(ctx.handle, S, sw, 0, sh, cn, X, Y, w, h, 1, 0, None, D),
        lambda: L.vp_remap_f32_dev(ctx.handle, S, sw, sw, sh, cn, X, Y, 0, h, 1, 0, None, D),
        lambda: L.vp_remap_f32_dev(ctx.handle, S, sw, sw, sh, cn, X, Y, w, -1, 1, 0, None, D),
        lambda: L.vp_remap_f32_dev(ctx.handle, S, 32768, 32768, 1, cn, X, Y, w, h, 1, 0, None, D),
        lambda: L.vp_remap_f32_dev(ctx.handle, S, sw, sw, 32768, cn, X, Y, w, h, 1, 0, None, D),
        lambda: L.vp_remap_f32_dev(ctx.handle, S, sw, sw, sh, cn, X, Y, w, h, 2, 0, None, D),
        lambda: L.vp_remap_f32_dev(ctx.handle, S, sw, sw, sh, cn, X, Y, w, h, 1, 4, None, D),
        lambda: L.vp_remap_f32_dev(ctx.handle, S, sw - 1, sw, sh, cn, X, Y, w, h, 1, 0, None, D),
        lambda: L.vp_remap_f32_dev(ctx.handle, S, sw, sw, sh, cn, X, Y, w, h, 1, 0, None, S),
        lambda: L.vp_remap_f32_dev(ctx.handle, S, sw, sw, sh, cn, X, Y, w, h, 1, 0, None, X),
        lambda: L.vp_remap_f32_dev(ctx.handle, S, sw, sw, sh, cn, X, Y, w, h, 1, 0, None, Y + 8),
        lambda: L.vp_remap_fixed_dev(ctx.handle, S, sw, sw, sh, cn, Q, F, w, h, 0, 0, None, D),          # nearest with a fraction plane
        lambda: L.vp_remap_fixed_dev(ctx.handle, S, sw, sw, sh, cn, Q, None, w, h, 1, 0, None, D),       # linear without one
        lambda: L.vp_remap_fixed_dev(ctx.handle, S, sw, sw, sh, cn, None, F, w, h, 1, 0, None, D),
        lambda: L.vp_remap_fixed_dev(ctx.handle, S, sw, sw, sh, cn, Q, F, w, h, 1, 0, None, Q),
        lambda: L.vp_remap_fixed_dev(ctx.handle, S, sw, sw, sh, cn, Q, F, w, h, 1, 0, None, F),
        lambda: L.vp_remap_fixed_dev(ctx.handle, S, sw, sw, sh, cn, Q, F, w, h, 1, 2, None, D),
        lambda: L.vp_remap_fixed_dev(ctx.handle, S, sw, sw, sh, 7, Q, F, w, h, 1, 0, None, D),
        lambda: L.vp_convert_maps_dev(ctx.handle, None, Y, w, h, 0, Q, F),
        lambda: L.vp_convert_maps_dev(ctx.handle, X, Y, w, h, 0, None, F),
        lambda: L.vp_convert_maps_dev(ctx.handle, X, Y, w, h, 0, Q, None),
        lambda: L.vp_convert_maps_dev(ctx.handle, X, Y, w, h, 1, Q, F),
        lambda: L.vp_convert_maps_dev(ctx.handle, X, Y, 0, h, 0, Q, F),
        lambda: L.vp_convert_maps_dev(ctx.handle, X, Y, w, h, 0, X, F),
        lambda: L.vp_convert_maps_dev(ctx.handle, X, Y, w, h, 0, Q, Q),
        lambda: L.vp_remap_u8(ctx.handle, None, sw, sh, cn, vp.ptr(mx), vp.ptr(my), w, h, 1, 0, None, vp.ptr(hd)),
        lambda: L.vp_remap_u8(ctx.handle, vp.ptr(hs), sw, sh, cn, None, vp.ptr(my), w, h, 1, 0, None, vp.ptr(hd)),
        lambda: L.vp_remap_u8(ctx.handle, vp.ptr(hs), sw, sh, cn, vp.ptr(mx), vp.ptr(my), w, h, 3, 0, None, vp.ptr(hd)),
        lambda: L.vp_remap_u8(ctx.handle, vp.ptr(hs), sw, sh, 9, vp.ptr(mx), vp.ptr(my), w, h, 1, 0, None, vp.ptr(hd)),
        lambda: L.vp_remap_u8(ctx.handle, vp.ptr(hs), 40000, sh, cn, vp.ptr(mx), vp.ptr(my), w, h, 1, 0, None, vp.ptr(hd)),
        lambda: L.vp_warp_perspective_dev(ctx.handle, S, sw, sw, sh, cn, None, 1, 0, None, D, w, h),
        lambda: L.vp_warp_perspective_dev(ctx.handle, S, sw, sw, sh, cn, vp.ptr(nan), 1, 0, None, D, w, h),
        lambda: L.vp_warp_perspective_dev(ctx.handle, S, sw, sw, sh, cn, vp.ptr(M), 2, 0, None, D, w, h),
        lambda: L.vp_warp_perspective_dev(ctx.handle, S, sw, sw, sh, cn, vp.ptr(M), 1, 2, None, D, w, h),
        lambda: L.vp_warp_perspective_dev(ctx.handle, S, sw - 1, sw, sh, cn, vp.ptr(M), 1, 0, None, D, w, h),
        lambda: L.vp_warp_perspective_dev(ctx.handle, S, sw, sw, sh, cn, vp.ptr(M), 1, 0, None, S, w, h),
        lambda: L.vp_warp_perspective_dev(ctx.handle, S, sw, sw, sh, cn, vp.ptr(M), 1, 0, None, D, w, 0),
        lambda: L.vp_warp_perspective_dev(ctx.handle, S, sw, sw, sh, 5, vp.ptr(M), 1, 0, None, D, w, h),
        lambda: L.vp_warp_perspective_u8(ctx.handle, vp.ptr(hs), sw, sh, cn, vp.ptr(M), 17 | 4, 0, None, vp.ptr(hd), w, h),
        lambda: L.vp_warp_perspective_u8(ctx.handle, vp.ptr(hs), 32768, sh, cn, vp.ptr(M), 1, 0, None, vp.ptr(hd), w, h),
        lambda: L.vp_warp_perspective_u8(ctx.handle, vp.ptr(hs), sw, sh, cn, vp.ptr(M), 1, 0, None, None, w, h),
    ]
    ctx.profile_begin(8)
    for i, call in enumerate(bad):
        assert call() == vp.ERR_INVALID, f"case {i} was not turned away"
    records = ctx.profile_end()
    assert len(records) == 0, "a kernel was launched for invalid arguments"
    assert (dst.host_copy() == 77).all() and (hd == 77).all(), "a destination was written"
    assert _same(xy.host_copy(), R.convert_maps_restate(mx, my)[0])
    # and the valid neighbours of those calls do run
    assert L.vp_remap_fixed_dev(ctx.handle, S, sw, sw, sh, cn, Q, F, w, h, 1, 0, None, D) == 0
    assert _same(dst.host_copy(), np.ascontiguousarray(img[:h, :w]))
