"""GPU suite for cv2.Sobel / Scharr / Laplacian / spatialGradient / convertScaleAbs (vp_deriv_*, vp_spatial_gradient_*,
vp_convert_scale_abs_*, vision.utils.transform, vision.cv2_facade).

Every comparison is byte for byte.  Expectations come from tests/deriv_restate.py (int64 correlation through explicit border index
maps, then the casts), never from the library under test.  The kernels' tile is DV_TB result bytes x DV_TH rows (read here from
csrc/vp_deriv_plan.h): the shapes are that tile exactly, one pixel more and less in each direction, the smallest images, and ragged
multi-channel ones; none had to be enlarged."""
import functools
import os
import re

import numpy as np
import pytest

import deriv_restate as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PLAN = open(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc", "vp_deriv_plan.h")).read()
TB = int(re.search(r"#define DV_TB (\d+)", _PLAN).group(1))
TH = int(re.search(r"#define DV_TH (\d+)", _PLAN).group(1))

TINY = [(1, 1, 1), (1, 9, 1), (9, 1, 1), (2, 2, 1), (3, 5, 1)]                                            # (h, w, cn)
TILE = [(TH, TB, 1), (TH + 1, TB, 1), (TH - 1, TB, 1), (TH, TB + 1, 1), (TH, TB - 1, 1)]
RAGGED = [(67, 35, 1), (67, 35, 3), (67, 35, 4), (301, 203, 3)]
BORDERS = [R.BORDER_REFLECT_101, R.BORDER_REPLICATE, R.BORDER_REFLECT, R.BORDER_CONSTANT]
DEPTHS = [R.CV_8U, R.CV_16S, R.CV_32F, R.CV_64F]
# (operator, dx, dy, ksize): every operator and ksize, every order pair at least once
OPS = [("sobel", 1, 0, 3), ("sobel", 0, 1, 3), ("sobel", 1, 1, 3), ("sobel", 2, 0, 3), ("sobel", 0, 2, 3), ("sobel", 2, 2, 3), ("sobel", 1, 0, 1), ("sobel", 0, 2, 1),
       ("sobel", 1, 1, 1), ("sobel", 1, 0, 5), ("sobel", 2, 1, 5), ("sobel", 0, 1, 7), ("sobel", 1, 0, 7), ("sobel", 2, 2, 7), ("sobel", 1, 0, -1), ("scharr", 1, 0, 3),
       ("scharr", 0, 1, 3), ("laplacian", 0, 0, 1), ("laplacian", 0, 0, 3), ("laplacian", 0, 0, 5), ("laplacian", 0, 0, 7)]


@functools.lru_cache(maxsize=None)
def _image(h, w, cn, seed=0):
    rng = np.random.default_rng(h * 1009 + w * 31 + cn * 7 + seed)
    a = rng.integers(0, 256, (h, w) if cn == 1 else (h, w, cn), dtype=np.uint8)
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def _expect(h, w, cn, op, dx, dy, k, dd, border, seed=0):
    img = _image(h, w, cn, seed)
    if op == "sobel":
        out = R.sobel_restate(img, dd, dx, dy, k, border)
    elif op == "scharr":
        out = R.scharr_restate(img, dd, dx, dy, border)
    else:
        out = R.laplacian_restate(img, dd, k, border)
    out.flags.writeable = False
    return out


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _dev(ctx, arr):
    from vision.devmat import DeviceMat
    return DeviceMat.from_host(ctx, arr)


def _facade(f, src, op, dx, dy, k, dd, border):
    if op == "sobel":
        return f.Sobel(src, dd, dx, dy, None, k, 1, 0, border)
    if op == "scharr":
        return f.Scharr(src, dd, dx, dy, None, 1, 0, border)
    return f.Laplacian(src, dd, None, k, 1, 0, border)


def _check(ctx, shape, op, dx, dy, k, dd, border):
    """the facade with a numpy source (the host entry) and with a DeviceMat source (the device entry) against the statement"""
    from vision import cv2_facade as f
    from vision.devmat import DeviceMat
    h, w, cn = shape
    img = _image(h, w, cn)
    exp = _expect(h, w, cn, op, dx, dy, k, dd, border)
    host = _facade(f, img, op, dx, dy, k, dd, border)
    assert type(host) is np.ndarray and _same(host, exp), (shape, op, dx, dy, k, dd, border, "host entry")
    src = _dev(ctx, img)
    out = _facade(f, src, op, dx, dy, k, dd, border)
    assert isinstance(out, DeviceMat) and out.dtype == exp.dtype and out.shape == exp.shape and not out.binary, (shape, op, dd)
    assert out._host is None and src._host is None, "a host copy was made"
    assert _same(np.asarray(out), exp), (shape, op, dx, dy, k, dd, border, "device entry")


@pytest.mark.parametrize("shape", TINY + TILE + RAGGED[:3])
def test_every_operator_and_ksize_at_every_shape(vp, shape):
    """int16 out, the default border; on the tiny shapes every border, where the index maps loop"""
    ctx = vp.default_context()
    for op, dx, dy, k in OPS:
        for border in (BORDERS if shape in TINY else BORDERS[:1]):
            _check(ctx, shape, op, dx, dy, k, R.CV_16S, border)


@pytest.mark.parametrize("dd", DEPTHS + [-1])
@pytest.mark.parametrize("border", BORDERS)
def test_every_depth_and_border(vp, dd, border):
    ctx = vp.default_context()
    for shape in ((67, 35, 3), (TH + 1, TB + 1, 1), (3, 5, 1)):
        for op, dx, dy, k in (("sobel", 1, 0, 3), ("sobel", 0, 1, 5), ("sobel", 1, 1, 7), ("scharr", 0, 1, 3), ("laplacian", 0, 0, 1), ("laplacian", 0, 0, 3),
                              ("laplacian", 0, 0, 5), ("laplacian", 0, 0, 7)):
            _check(ctx, shape, op, dx, dy, k, dd, border | (R.BORDER_ISOLATED if shape[2] == 3 else 0))


def test_bgr_image_of_several_tiles(vp):
    ctx = vp.default_context()
    for op, dx, dy, k, dd in (("sobel", 1, 0, 3, R.CV_16S), ("sobel", 0, 1, 5, R.CV_32F), ("sobel", 2, 0, 7, R.CV_8U), ("laplacian", 0, 0, 3, R.CV_64F),
                              ("laplacian", 0, 0, 7, R.CV_16S), ("scharr", 1, 0, 3, R.CV_8U)):
        _check(ctx, RAGGED[3], op, dx, dy, k, dd, R.BORDER_REFLECT_101)


def test_aligned_rows_take_the_vector_stores(vp):
    """w * cn a multiple of 8 (and of 16 / sizeof): every lane stores 8 results at once; 2 channels ride along"""
    ctx = vp.default_context()
    for shape in ((TH + 3, TB + 64, 1), (21, 40, 2), (21, 176, 3), (20, 64, 4)):
        for dd in DEPTHS:
            _check(ctx, shape, "sobel", 1, 0, 3, dd, R.BORDER_REFLECT_101)
            _check(ctx, shape, "laplacian", 0, 0, 1, dd, R.BORDER_REPLICATE)
            _check(ctx, shape, "laplacian", 0, 0, 5, dd, R.BORDER_REFLECT)


def test_strided_source_with_an_odd_byte_offset_through_the_c_abi(vp):
    """A column window of a wider device image (src_stride > w * cn, first byte at an odd address, a stride that is no multiple of 4:
    every row starts at another phase) gives the bytes of the packed case."""
    from vision.devmat import DeviceMat
    ctx = vp.default_context()
    L = vp.lib()
    rng = np.random.default_rng(5)
    h, x0, w = 45, 31, 67
    for cn, W in ((1, 200), (3, 200), (4, 201), (1, 201), (3, 333)):
        wide = rng.integers(0, 256, (h, W, cn), dtype=np.uint8)
        win = np.ascontiguousarray(wide[:, x0:x0 + w])
        buf = _dev(ctx, wide)
        assert cn % 2 == 0 or (buf.dev_ptr + x0 * cn) % 2 == 1
        for op, code, dx, dy, k, dd, border in (("sobel", vp.DERIV_SOBEL, 1, 0, 3, R.CV_16S, R.BORDER_REFLECT_101), ("sobel", vp.DERIV_SOBEL, 0, 1, 7, R.CV_32F, R.BORDER_REFLECT),
                                                ("scharr", vp.DERIV_SCHARR, 1, 0, 3, R.CV_8U, R.BORDER_REPLICATE), ("laplacian", vp.DERIV_LAPLACIAN, 0, 0, 1, R.CV_16S, R.BORDER_CONSTANT),
                                                ("laplacian", vp.DERIV_LAPLACIAN, 0, 0, 5, R.CV_64F, R.BORDER_REFLECT_101)):
            out = DeviceMat(ctx, (h, w, cn), R.DTYPES[dd])
            vp.check(L.vp_deriv_dev(ctx.handle, buf.dev_ptr + x0 * cn, W * cn, w, h, cn, code, dx, dy, k, dd, border, out.dev_ptr), ctx.handle)
            if op == "sobel":
                exp = R.sobel_restate(win, dd, dx, dy, k, border)
            elif op == "scharr":
                exp = R.scharr_restate(win, dd, dx, dy, border)
            else:
                exp = R.laplacian_restate(win, dd, k, border)
            assert _same(np.asarray(out), exp), (cn, W, op, k)
        if cn == 1:
            gx, gy = DeviceMat(ctx, (h, w), np.int16), DeviceMat(ctx, (h, w), np.int16)
            vp.check(L.vp_spatial_gradient_dev(ctx.handle, buf.dev_ptr + x0, W, w, h, 3, R.BORDER_REPLICATE, gx.dev_ptr, gy.dev_ptr), ctx.handle)
            ex, ey = R.spatial_gradient_restate(win[:, :, 0], R.BORDER_REPLICATE)
            assert _same(np.asarray(gx), ex) and _same(np.asarray(gy), ey), W


def test_host_entries_through_the_c_abi(vp):
    ctx = vp.default_context()
    L = vp.lib()
    img = _image(67, 35, 3)
    out = np.empty(img.shape, np.float32)
    vp.check(L.vp_deriv_u8(ctx.handle, vp.ptr(img), 35, 67, 3, vp.DERIV_SOBEL, 1, 1, 5, R.CV_32F, R.BORDER_REFLECT, vp.ptr(out)), ctx.handle)
    assert _same(out, R.sobel_restate(img, R.CV_32F, 1, 1, 5, R.BORDER_REFLECT))
    grey = _image(67, 35, 1)
    gx, gy = np.empty(grey.shape, np.int16), np.empty(grey.shape, np.int16)
    vp.check(L.vp_spatial_gradient_u8(ctx.handle, vp.ptr(grey), 35, 67, 3, R.BORDER_REFLECT_101, vp.ptr(gx), vp.ptr(gy)), ctx.handle)
    ex, ey = R.spatial_gradient_restate(grey)
    assert _same(gx, ex) and _same(gy, ey)
    vals = np.arange(-40000, 40000, 7).astype(np.int16)
    dst = np.empty(vals.shape, np.uint8)
    vp.check(L.vp_convert_scale_abs_u8(ctx.handle, vp.ptr(vals), R.CV_16S, vals.size, vp.ptr(dst)), ctx.handle)
    assert _same(dst, R.convert_scale_abs_restate(vals))


def test_rejected_device_calls_launch_nothing(vp):
    from vision.devmat import DeviceMat
    ctx = vp.default_context()
    L = vp.lib()
    h, w = 20, 64
    buf = DeviceMat(ctx, (4 * h, w))
    before = np.arange(4 * h * w, dtype=np.uint32).astype(np.uint8).reshape(4 * h, w)
    vp.check(L.vp_memcpy_h2d(ctx.handle, buf.dev_ptr, before.ctypes.data, before.nbytes), ctx.handle)
    p = buf.dev_ptr
    S = (vp.DERIV_SOBEL, 1, 0, 3)
    assert L.vp_deriv_dev(ctx.handle, p, w, w, h, 1, *S, R.CV_8U, 4, p + 16) == vp.ERR_INVALID                    # overlap
    assert L.vp_deriv_dev(ctx.handle, p, w, w, h, 1, *S, R.CV_16S, 4, p + h * w - 2) == vp.ERR_INVALID            # the int16 result reaches back into src
    assert L.vp_deriv_dev(ctx.handle, p, w, w, h, 1, *S, R.CV_16S, 4, p + h * w + 1) == vp.ERR_INVALID            # an int16 plane at an odd address
    assert L.vp_deriv_dev(ctx.handle, p, w - 1, w, h, 1, *S, R.CV_8U, 4, p + h * w) == vp.ERR_INVALID             # stride below the row
    assert L.vp_deriv_dev(ctx.handle, p, w, w, h, 1, *S, R.CV_8U, 3, p + h * w) == vp.ERR_INVALID                 # BORDER_WRAP
    assert L.vp_deriv_dev(ctx.handle, p, w, w, h, 1, vp.DERIV_SOBEL, 0, 0, 3, R.CV_8U, 4, p + h * w) == vp.ERR_INVALID
    assert L.vp_deriv_dev(ctx.handle, p, w, w, h, 1, 3, 1, 0, 3, R.CV_16S, 4, p + h * w) == vp.ERR_INVALID          # no such operator
    assert L.vp_spatial_gradient_dev(ctx.handle, p, w, w, h, 3, 4, p + h * w, p + h * w + 2) == vp.ERR_INVALID    # the planes overlap
    assert L.vp_spatial_gradient_dev(ctx.handle, p, w, w, h, 3, 2, p + h * w, p + 3 * h * w) == vp.ERR_INVALID    # BORDER_REFLECT
    assert L.vp_spatial_gradient_dev(ctx.handle, p, w, w, h, 5, 4, p + h * w, p + 3 * h * w) == vp.ERR_INVALID    # ksize
    assert L.vp_convert_scale_abs_dev(ctx.handle, p, R.CV_16S, h * w, p + 2 * h * w - 1) == vp.ERR_INVALID
    assert L.vp_convert_scale_abs_dev(ctx.handle, p + 1, R.CV_16S, h * w, p + 2 * h * w + 2) == vp.ERR_INVALID
    assert L.vp_convert_scale_abs_dev(ctx.handle, p, 4, h * w, p + 3 * h * w) == vp.ERR_INVALID
    ctx.synchronize()
    after = np.empty_like(before)
    vp.check(L.vp_memcpy_d2h(ctx.handle, after.ctypes.data, buf.dev_ptr, after.nbytes), ctx.handle)
    assert np.array_equal(after, before), "a rejected call wrote to the image"
    assert L.vp_deriv_dev(ctx.handle, p, w, w, h, 1, *S, R.CV_8U, 4, p + h * w) == vp.OK                          # apart: accepted
    ctx.synchronize()


def test_ksize7_step_edge_saturates_int16(vp):
    from vision import cv2_facade as f
    ctx = vp.default_context()
    step = np.zeros((40, TB + 40), np.uint8)
    step[:, TB - 3:] = 255                                       # the edge sits on a tile seam
    for img in (step, np.ascontiguousarray(step[:, ::-1]), np.ascontiguousarray(step.T)):
        for dx, dy in ((1, 0), (0, 1)):
            exp = R.sobel_restate(img, R.CV_16S, dx, dy, 7)
            out = f.Sobel(_dev(ctx, img), f.CV_16S, dx, dy, ksize=7)
            assert _same(np.asarray(out), exp)
            assert _same(f.Sobel(img, f.CV_16S, dx, dy, ksize=7), exp)
            raw = R.correlate(img, np.outer(*R.sobel_kernel(dx, dy, 7)), R.BORDER_REFLECT_101)
            assert _same(np.asarray(f.Sobel(_dev(ctx, img), f.CV_32F, dx, dy, ksize=7)), raw.astype(np.float32))
    exp = R.sobel_restate(step, R.CV_16S, 1, 0, 7)
    assert exp.max() == 32767 and R.sobel_restate(np.ascontiguousarray(step[:, ::-1]), R.CV_16S, 1, 0, 7).min() == -32768
    u = f.Sobel(_dev(ctx, np.ascontiguousarray(step[:, ::-1])), f.CV_8U, 1, 0)
    assert not np.asarray(u).any(), "negative responses clamp to 0 in uint8"


@pytest.mark.parametrize("border", [R.BORDER_REFLECT_101, R.BORDER_REPLICATE])
def test_spatial_gradient_equals_the_two_sobels(vp, border):
    from vision import cv2_facade as f
    from vision.devmat import DeviceMat
    ctx = vp.default_context()
    for h, w in ((1, 1), (3, 5), (67, 35), (TH + 1, TB + 1), (TH, TB)):
        img = _image(h, w, 1)
        ex, ey = R.spatial_gradient_restate(img, border)
        gx, gy = f.spatialGradient(img, None, None, 3, border)
        assert type(gx) is np.ndarray and _same(gx, ex) and _same(gy, ey), (h, w, "host")
        src = _dev(ctx, img)
        dgx, dgy = f.spatialGradient(src, borderType=border)
        assert isinstance(dgx, DeviceMat) and isinstance(dgy, DeviceMat) and dgx._host is None and dgy._host is None and src._host is None
        sx, sy = f.Sobel(src, f.CV_16S, 1, 0, ksize=3, borderType=border), f.Sobel(src, f.CV_16S, 0, 1, ksize=3, borderType=border)
        assert _same(np.asarray(dgx), ex) and _same(np.asarray(dgy), ey), (h, w, "device")
        assert _same(np.asarray(sx), ex) and _same(np.asarray(sy), ey), (h, w, "the two Sobels")


def test_convert_scale_abs_values(vp):
    from vision import cv2_facade as f
    from vision.devmat import DeviceMat
    ctx = vp.default_context()
    rng = np.random.default_rng(9)
    edge16 = np.array([-32768, -32767, -257, -256, -255, -254, -1, 0, 1, 254, 255, 256, 257, 32767], np.int16)
    ties = np.array([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 253.5, 254.5, 255.5, -254.5, -255.5, 0.49999997, 0.50000006, 2.4999998, 254.49998, 1e9, -1e9,
                     3e38, np.inf, -np.inf, np.nan, -0.0, 255.0, 256.0], np.float32)
    for n in (1, 15, 16, 17, 1000, 4099):              # below one 16-byte group, heads and tails
        for src in (np.resize(edge16, n), rng.integers(-32768, 32768, n).astype(np.int16), np.resize(ties, n), np.resize(ties, n).astype(np.float64),
                    (rng.random(n) * 600 - 300).astype(np.float32), rng.random(n) * 600 - 300, rng.integers(0, 256, n, dtype=np.uint8)):
            img = src.reshape(1, n)
            exp = R.convert_scale_abs_restate(img)
            host = f.convertScaleAbs(img)
            assert type(host) is np.ndarray and _same(host, exp), (n, src.dtype, "host")
            d = _dev(ctx, img)
            out = f.convertScaleAbs(d)
            assert isinstance(out, DeviceMat) and out.dtype == np.uint8 and out._host is None and d._host is None
            assert _same(np.asarray(out), exp), (n, src.dtype, "device")
    # an int16 plane that does not start at a multiple of 16 bytes: element loads into the same stores
    from vision.devmat import DeviceMat as DM
    vals = rng.integers(-400, 400, 5000).astype(np.int16)
    buf = _dev(ctx, vals)
    out = DM(ctx, (4990,))
    vp.check(vp.lib().vp_convert_scale_abs_dev(ctx.handle, buf.dev_ptr + 6, R.CV_16S, 4990, out.dev_ptr), ctx.handle)
    assert _same(np.asarray(out), R.convert_scale_abs_restate(vals[3:4993]))
    img3 = rng.integers(-300, 300, (37, 29, 3)).astype(np.int16)
    assert _same(np.asarray(f.convertScaleAbs(_dev(ctx, img3))), R.convert_scale_abs_restate(img3))


def test_gradient_chain_stays_on_the_device(vp):
    """Sobel -> convertScaleAbs -> addWeighted -> threshold: device images throughout, nothing visits the host"""
    from vision import cv2_facade as f
    from vision.devmat import DeviceMat
    ctx = vp.default_context()
    img = _image(67, 35, 1, seed=3)
    src = _dev(ctx, img)
    gx = f.Sobel(src, f.CV_16S, 1, 0)
    gy = f.Sobel(src, f.CV_16S, 0, 1)
    ax, ay = f.convertScaleAbs(gx), f.convertScaleAbs(gy)
    mix = f.addWeighted(ax, 0.5, ay, 0.5, 0)
    _, mask = f.threshold(mix, 60, 255, f.THRESH_BINARY)
    stages = (src, gx, gy, ax, ay, mix, mask)
    assert all(isinstance(m, DeviceMat) for m in stages)
    assert gx.dtype == np.int16 and ax.dtype == np.uint8 and mask.dtype == np.uint8
    result = mask.host_copy()
    assert all(m._host is None for m in stages), "an input or an intermediate visited the host"
    ex, ey = R.sobel_restate(img, R.CV_16S, 1, 0), R.sobel_restate(img, R.CV_16S, 0, 1)
    acc = R.convert_scale_abs_restate(ex).astype(np.float64) * 0.5 + R.convert_scale_abs_restate(ey).astype(np.float64) * 0.5
    want = np.where(np.clip(np.rint(acc), 0, 255) > 60, 255, 0).astype(np.uint8)
    assert _same(result, want)


def test_dst_receives_the_result(vp):
    from vision import cv2_facade as f
    img = _image(67, 35, 3)
    exp = R.sobel_restate(img, R.CV_16S, 1, 0)
    dst = np.zeros(img.shape, np.int16)
    assert f.Sobel(img, f.CV_16S, 1, 0, dst) is dst and _same(dst, exp)
    dst = np.zeros(img.shape, np.float32)
    assert f.Laplacian(img, f.CV_32F, dst, 3) is dst and _same(dst, R.laplacian_restate(img, R.CV_32F, 3))
    dst = np.zeros(img.shape, np.uint8)
    assert f.Scharr(img, -1, 0, 1, dst) is dst and _same(dst, R.scharr_restate(img, R.CV_8U, 0, 1))
    dst = np.zeros(img.shape, np.uint8)
    assert f.convertScaleAbs(exp, dst) is dst and _same(dst, R.convert_scale_abs_restate(exp))
    grey = _image(67, 35, 1)
    dx, dy = np.zeros(grey.shape, np.int16), np.zeros(grey.shape, np.int16)
    gx, gy = f.spatialGradient(grey, dx, dy)
    ex, ey = R.spatial_gradient_restate(grey)
    assert gx is dx and gy is dy and _same(dx, ex) and _same(dy, ey)
    wrong = np.zeros(img.shape, np.uint8)                      # another type: cv2 reallocates, the result is returned
    out = f.Sobel(img, f.CV_16S, 1, 0, wrong)
    assert out is not wrong and _same(out, exp) and not wrong.any()


def test_mirror_names(vp):
    from vision.devmat import DeviceMat
    from vision.utils import transform as t
    ctx = vp.default_context()
    img = _image(67, 35, 3)
    assert _same(t.sobel(img, 1, 0), R.sobel_restate(img, R.CV_16S, 1, 0))
    assert _same(t.scharr(img, 0, 1, vp.DEPTH_32F), R.scharr_restate(img, R.CV_32F, 0, 1))
    assert _same(t.laplacian(img, 5, vp.DEPTH_8U, vp.BORDER_REPLICATE), R.laplacian_restate(img, R.CV_8U, 5, R.BORDER_REPLICATE))
    out = t.sobel(_dev(ctx, img), 0, 1, 5, vp.DEPTH_64F)
    assert isinstance(out, DeviceMat) and out.dtype == np.float64 and _same(np.asarray(out), R.sobel_restate(img, R.CV_64F, 0, 1, 5))
    grey = _image(67, 35, 1)
    gx, gy = t.spatial_gradient(_dev(ctx, grey.reshape(67, 35, 1)))
    ex, ey = R.spatial_gradient_restate(grey)
    assert _same(np.asarray(gx), ex) and _same(np.asarray(gy), ey)
