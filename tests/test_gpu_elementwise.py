"""GPU suite for the element-wise operators on device images (csrc/vp_elementwise.hip): the DeviceMat operators & | ^ ~, the cv2
stand-in's bitwise_* / add / subtract / absdiff / LUT / split / merge / extractChannel / countNonZero, and the preprocessor's channel
bias, which with them never leaves the device.

Every comparison is bit-exact against a numpy statement written here (and the CPU oracle for the blur / dilate that follow)."""
import ctypes as C

import numpy as np
import pytest

import frames as F

pytestmark = pytest.mark.gpu

FLAT_N = [1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097]


def _dev(ctx, arr):
    from vision.devmat import DeviceMat
    return DeviceMat.from_host(ctx, arr)


def _resident(*mats):
    from vision.devmat import DeviceMat
    for m in mats:
        assert isinstance(m, DeviceMat), type(m)
        assert m._host is None, "an image was downloaded although nothing read it"


def _get(m):
    """Contents of a result that must have stayed on the device."""
    _resident(m)
    return m.host_copy()


def _offset_view(ctx, arr, offset):
    """`arr` as a device image that starts `offset` bytes into its allocation (a plane of a frame inside a shared buffer)."""
    from vision.devmat import DeviceMat
    flat = np.zeros(offset + arr.size + 64, np.uint8)
    flat[offset:offset + arr.size] = arr.ravel()
    base = _dev(ctx, flat)
    m = DeviceMat.over_buffer(ctx, base._buf, offset, arr.shape, np.uint8)
    assert m.dev_ptr % 16 == offset % 16
    return m


def _sat(acc):
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def _shapes():
    return [(1, n) for n in FLAT_N] + [(1, n, 3) for n in FLAT_N] + [(3, 67), (5, 67, 3)]


def _pair(rng, shape):
    a = rng.integers(0, 256, shape, dtype=np.uint8)
    b = rng.integers(0, 256, shape, dtype=np.uint8)
    k = min(a.size, 8)
    a.ravel()[:k] = [0, 255, 0, 255, 1, 254, 128, 127][:k]                  # both ends of the range on both sides
    b.ravel()[:k] = [0, 255, 255, 0, 254, 1, 127, 128][:k]
    return a, b


def _all_ops(f, da, db, a, b, lut1, lutc):
    """(result, expectation) of every image-with-image operator, and of the tables."""
    ai, bi = a.astype(np.int32), b.astype(np.int32)
    out = [(da & db, a & b), (da | db, a | b), (da ^ db, a ^ b), (~da, ~a), (f.bitwise_xor(da, db), a ^ b), (f.bitwise_not(da), ~a),
           (f.add(da, db), np.clip(ai + bi, 0, 255)), (f.subtract(da, db), np.clip(ai - bi, 0, 255)), (f.absdiff(da, db), np.abs(ai - bi)),
           (f.LUT(da, lut1), lut1[a])]
    if a.ndim == 3:
        out.append((f.LUT(da, lutc), np.stack([lutc[:, c][a[:, :, c]] for c in range(a.shape[2])], axis=2)))
    return out


def test_flat_sizes_bitwise_arith_and_lut(vp):
    from vision import cv2_facade as f
    ctx = vp.default_context()
    rng = np.random.default_rng(1)
    lut1 = rng.integers(0, 256, 256, dtype=np.uint8)
    lutc = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    for shape in _shapes() + [(1080, 1920, 3)]:
        a, b = _pair(rng, shape)
        da, db = _dev(ctx, a), _dev(ctx, b)
        for got, exp in _all_ops(f, da, db, a, b, lut1, lutc):
            assert np.array_equal(_get(got), exp), shape
        _resident(da, db)


def test_operands_at_an_offset_and_from_numpy(vp):
    """Every operator once with an operand that does not start at a 16-byte boundary (a plane inside a shared allocation), with a
    plane bgr_to_lab made, and with a numpy operand, which is uploaded."""
    from vision import cv2_facade as f
    from vision.utils.color import bgr_to_lab
    ctx = vp.default_context()
    rng = np.random.default_rng(2)
    lut1 = rng.integers(0, 256, 256, dtype=np.uint8)
    lutc = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    for shape in ((45, 67), (9, 21, 3)):
        a, b = _pair(rng, shape)
        for off_a, off_b in ((3, 0), (0, 5), (7, 7), (1, 14)):
            da, db = _offset_view(ctx, a, off_a), _offset_view(ctx, b, off_b)
            for got, exp in _all_ops(f, da, db, a, b, lut1, lutc):
                assert np.array_equal(_get(got), exp), (shape, off_a, off_b)
        for got, exp in _all_ops(f, _dev(ctx, a), b, a, b, lut1, lutc):        # numpy on the right ...
            assert np.array_equal(_get(got), exp)
        ai, bi = a.astype(np.int32), b.astype(np.int32)
        for got, exp in ((a & _dev(ctx, b), a & b), (a | _dev(ctx, b), a | b), (a ^ _dev(ctx, b), a ^ b),      # ... and on the left
                         (f.subtract(a, _dev(ctx, b)), np.clip(ai - bi, 0, 255)), (f.add(a, _dev(ctx, b)), np.clip(ai + bi, 0, 255))):
            assert np.array_equal(_get(got), exp)
    img = F.s1_buoy(3, 67, 45)
    lab, planes = bgr_to_lab(_dev(ctx, img))
    pa, pb = planes[1], planes[2]
    _resident(pa, pb)
    ha, hb = pa.host_copy(), pb.host_copy()
    for got, exp in _all_ops(f, pa, pb, ha, hb, lut1, lutc):
        assert np.array_equal(_get(got), exp)
    # split planes share one allocation: plane c starts c * 256-byte-rounded plane sizes in
    s0, s1, s2 = f.split(lab)
    assert s0._buf is s1._buf is s2._buf and (s1._off, s2._off) == (3072, 6144) and s1.dev_ptr % 256 == 0
    for got, exp in _all_ops(f, s1, s2, ha, hb, lut1, lutc):
        assert np.array_equal(_get(got), exp)


def test_bitwise_with_scalars_and_masks(vp):
    from vision import cv2_facade as f
    ctx = vp.default_context()
    rng = np.random.default_rng(3)
    for shape in ((5, 67), (5, 67, 3), (1, 4097), (2, 64, 3)):
        a, b = _pair(rng, shape)
        da, db = _dev(ctx, a), _dev(ctx, b)
        for s in (0, 1, 0xF0, 255):
            for got, exp in ((da & s, a & s), (da | s, a | s), (da ^ s, a ^ s), (s & da, a & s), (s | da, a | s), (s ^ da, a ^ s),
                             (da & np.uint8(s), a & np.uint8(s)), (f.bitwise_and(da, s), a & s), (f.bitwise_or(s, da), a | s)):
                assert exp.dtype == np.uint8 and np.array_equal(_get(got), exp), (shape, s)
        m = rng.choice(np.array([0, 7, 255], np.uint8), shape[:2])          # a mask byte that is neither 0 nor 255 counts as set
        keep = (m != 0) if a.ndim == 2 else (m != 0)[:, :, None]
        for dm in (_dev(ctx, m), m, _offset_view(ctx, m, 3)):
            for got, exp in ((f.bitwise_and(da, db, mask=dm), np.where(keep, a & b, 0)), (f.bitwise_or(da, db, mask=dm), np.where(keep, a | b, 0)),
                             (f.bitwise_xor(da, db, mask=dm), np.where(keep, a ^ b, 0)), (f.bitwise_not(da, mask=dm), np.where(keep, ~a, 0)),
                             (f.bitwise_and(da, da, mask=dm), np.where(keep, a, 0)), (f.bitwise_and(_offset_view(ctx, a, 5), db, mask=dm), np.where(keep, a & b, 0))):
                assert np.array_equal(_get(got), exp), shape
    # operands the device path does not take go through numpy, as before
    a, b = _pair(rng, (4, 6))
    da = _dev(ctx, a)
    for got, exp in ((da & np.int32(256), a & np.int32(256)), (da & np.int16(-1), a & np.int16(-1)), (da & b[:1], a & b[:1]), (da & True, a & True), (da + b, a + b), (da < b, a < b)):
        assert type(got) is np.ndarray and got.dtype == exp.dtype and np.array_equal(got, exp)


def test_c_abi_destination_may_be_a_source(vp):
    """vp_bitwise_u8_dev / vp_arith_u8_dev / vp_lut_u8_dev with dst == a and dst == b, dst at every alignment; a partial overlap is refused."""
    from vision import _vp
    ctx = vp.default_context()
    lib = vp.lib()
    rng = np.random.default_rng(4)
    lut = rng.integers(0, 256, 256, dtype=np.uint8)
    made = C.c_int(0)
    for n in (1, 17, 64, 4097):
        for off in (0, 1, 9):
            a, b = _pair(rng, (1, n))
            ai, bi = a.astype(np.int32), b.astype(np.int32)
            for alias_b in (False, True):
                for op, exp in ((_vp.BITWISE_AND, a & b), (_vp.BITWISE_OR, a | b), (_vp.BITWISE_XOR, a ^ b), (_vp.BITWISE_NOT, ~a)):
                    da, db = _offset_view(ctx, a, off), _offset_view(ctx, b, off)
                    dst = db if (alias_b and op != _vp.BITWISE_NOT) else da
                    vp.check(lib.vp_bitwise_u8_dev(ctx.handle, op, da.dev_ptr, db.dev_ptr, 0, None, 1, n, dst.dev_ptr, 0, None, C.byref(made)), ctx.handle)
                    assert np.array_equal(dst.host_copy(), exp) and made.value == 0, (n, off, op, alias_b)
                for op, exp in ((_vp.ARITH_ADD, np.clip(ai + bi, 0, 255)), (_vp.ARITH_SUB, np.clip(ai - bi, 0, 255)), (_vp.ARITH_ABSDIFF, np.abs(ai - bi))):
                    da, db = _offset_view(ctx, a, off), _offset_view(ctx, b, off)
                    dst = db if alias_b else da
                    vp.check(lib.vp_arith_u8_dev(ctx.handle, op, da.dev_ptr, db.dev_ptr, n, dst.dev_ptr), ctx.handle)
                    assert np.array_equal(dst.host_copy(), exp), (n, off, op, alias_b)
            da = _offset_view(ctx, a, off)
            vp.check(lib.vp_lut_u8_dev(ctx.handle, da.dev_ptr, n, 1, lut.ctypes.data, da.dev_ptr), ctx.handle)
            assert np.array_equal(da.host_copy(), lut[a])
    a, b = _pair(rng, (1, 64))
    da, db = _dev(ctx, a), _dev(ctx, b)
    assert lib.vp_bitwise_u8_dev(ctx.handle, _vp.BITWISE_AND, da.dev_ptr, db.dev_ptr, 0, None, 1, 32, da.dev_ptr + 8, 0, None, None) != 0
    assert lib.vp_arith_u8_dev(ctx.handle, _vp.ARITH_ADD, da.dev_ptr, db.dev_ptr, 32, db.dev_ptr + 16) != 0
    assert lib.vp_bitwise_u8_dev(ctx.handle, _vp.BITWISE_AND, da.dev_ptr, None, 256, None, 1, 32, da.dev_ptr, 0, None, None) != 0
    assert lib.vp_bitwise_u8_dev(ctx.handle, 4, da.dev_ptr, db.dev_ptr, 0, None, 1, 32, da.dev_ptr, 0, None, None) != 0
    assert np.array_equal(da.host_copy(), a) and np.array_equal(db.host_copy(), b)


@pytest.mark.parametrize("w,h", [(64, 3), (128, 5), (65, 4)])
def test_masks_stay_masks_and_bring_their_bit_plane(vp, oracle, w, h):
    from vision.utils.color import range_threshold
    from vision.utils.feature import outer_contours
    from vision.utils.transform import dilate, rect_kernel
    ctx = vp.default_context()
    rng = np.random.default_rng(w)
    yy, xx = np.mgrid[0:h, 0:w]
    g1 = ((xx // 5 + yy) % 3 * 100 + rng.integers(0, 40, (h, w))).astype(np.uint8)
    g2 = ((xx // 7 + 2 * yy) % 4 * 70 + rng.integers(0, 40, (h, w))).astype(np.uint8)
    na, nb = np.where(g1 >= 100, 255, 0).astype(np.uint8), np.where((g2 >= 60) & (g2 <= 200), 255, 0).astype(np.uint8)
    k3 = np.ones((3, 3), np.uint8)
    for name, exp in (("and", na & nb), ("or", na | nb), ("xor", na ^ nb), ("not", ~na), ("and255", na & 255), ("xor255", na ^ 255)):
        a, b = range_threshold(g1, 100, 255), range_threshold(g2, 60, 200)
        _resident(a, b)
        assert a.binary is True and b.binary is True
        c = {"and": lambda: a & b, "or": lambda: a | b, "xor": lambda: a ^ b, "not": lambda: ~a, "and255": lambda: a & 255, "xor255": lambda: a ^ 255}[name]()
        _resident(c)
        assert c.binary is True and c.shape == (h, w)
        bits = c.bit_plane(ctx)                            # (launches a result that was waiting)
        if w % 64 == 0:
            assert bits is not None and c._bits is bits
            words = np.empty((h, w // 64), np.uint64)
            vp.check(vp.lib().vp_memcpy_d2h(ctx.handle, words.ctypes.data, bits.ptr, words.nbytes), ctx.handle)
            assert np.array_equal(words.view(np.uint8).reshape(h, w // 8), np.packbits(exp != 0, axis=1, bitorder="little")), name
        else:
            assert bits is None and c._bits is None
        assert np.array_equal(_get(c), exp), name
        got, ref = outer_contours(c), outer_contours(_dev(ctx, np.ascontiguousarray(exp)))
        assert len(got) == len(ref) and all(np.array_equal(x, y) for x, y in zip(got, ref)), name
        d = dilate(c, rect_kernel(3))
        _resident(c, d)
        assert d.binary is True and np.array_equal(_get(d), oracle.morph(oracle.DILATE, np.ascontiguousarray(exp), k3)), name
    a = range_threshold(g1, 100, 255)
    assert (a & 0xF0).binary is False and (a & _dev(ctx, g2)).binary is False and (a | 1).binary is False
    assert np.array_equal(_get(a & _dev(ctx, g2)), na & g2)
    # a fresh contour pass of a deferred result takes the bit plane of the launch it triggers
    c = range_threshold(g1, 100, 255) & range_threshold(g2, 60, 200)
    got, ref = outer_contours(c), outer_contours(_dev(ctx, na & nb))
    assert len(got) == len(ref) and all(np.array_equal(x, y) for x, y in zip(got, ref))
    assert (c._bits is not None) == (w % 64 == 0)


def test_deferral_and_modes(vp):
    from vision import devmat
    ctx = vp.default_context()
    rng = np.random.default_rng(7)
    na, nb = _pair(rng, (6, 70))
    a, b = _dev(ctx, na), _dev(ctx, nb)
    assert devmat.defer_enabled()
    c = a & b
    n = ~a
    assert c._pending is not None and n._pending is not None
    a[0, 0] = 255 - na[0, 0]                               # a host-side write to an input: what waits for it runs first
    assert c._pending is None and n._pending is None
    assert np.array_equal(np.asarray(c), na & nb) and np.array_equal(np.asarray(n), ~na)
    na2 = na.copy()
    na2[0, 0] = 255 - na[0, 0]
    assert np.array_equal(_get(a & b), na2 & nb)           # the next operator sees the write
    view = np.asarray(b)                                   # a writable alias is out: launched at the call
    c = a & b
    assert c._pending is None and view is not None and np.array_equal(c.host_copy(), na2 & nb)
    devmat.set_defer(False)
    try:
        a, b = _dev(ctx, na), _dev(ctx, nb)
        c = a | b
        assert c._pending is None and c._buf is not None and np.array_equal(_get(c), na | nb)
    finally:
        devmat.set_defer(True)
    devmat.set_lazy(False)
    try:
        a, b = _dev(ctx, na), _dev(ctx, nb)
        for got, exp in ((a & b, na & nb), (a | nb, na | nb), (na ^ b, na ^ nb), (~a, ~na), (a & 15, na & 15)):
            assert type(got) is np.ndarray and np.array_equal(got, exp)
    finally:
        devmat.set_lazy(True)


def test_arithmetic_with_scalars(vp):
    from vision import cv2_facade as f
    ctx = vp.default_context()
    rng = np.random.default_rng(8)
    bgr = rng.integers(0, 256, (9, 37, 3), dtype=np.uint8)
    bgr.ravel()[:256] = np.arange(256)
    gray = np.ascontiguousarray(bgr[:, :, 1])
    for img in (bgr, gray):
        x = img.astype(np.float64)
        d = _dev(ctx, img)
        for s in (-300, -20, -0.5, 0, 0.5, 1.5, 10, 255, 300):
            for got, exp in ((f.add(d, s), _sat(x + float(s))), (f.add(s, d), _sat(x + float(s))), (f.subtract(d, s), _sat(x - float(s))),
                             (f.subtract(s, d), _sat(float(s) - x)), (f.absdiff(d, s), _sat(np.abs(x - float(s))))):
                assert np.array_equal(_get(got), exp), s
    d = _dev(ctx, bgr)
    x = bgr.astype(np.float64)
    t = np.array((1, -2, 300), np.float64)
    assert np.array_equal(_get(f.add((1, -2, 300), d)), _sat(x + t))
    assert np.array_equal(_get(f.subtract((1, -2, 300), d)), _sat(t - x)) and np.array_equal(_get(f.subtract(d, (1, -2, 300))), _sat(x - t))
    four = rng.integers(0, 256, (3, 7, 4), dtype=np.uint8)
    assert np.array_equal(_get(f.add(_dev(ctx, four), (5, -5, 0.5, 200))), _sat(four.astype(np.float64) + np.array((5, -5, 0.5, 200))))
    dst = np.empty_like(bgr)
    assert f.add(d, 7, dst) is dst and np.array_equal(dst, _sat(x + 7.0))


def test_lut(vp):
    from vision import cv2_facade as f
    ctx = vp.default_context()
    rng = np.random.default_rng(9)
    for cn in (1, 2, 3, 4):
        img = rng.integers(0, 256, (5, 67, cn), dtype=np.uint8)
        img.ravel()[:256] = np.arange(256)
        one = rng.integers(0, 256, 256, dtype=np.uint8)
        per = rng.integers(0, 256, (256, cn), dtype=np.uint8)
        exp_per = np.stack([per[:, c][img[:, :, c]] for c in range(cn)], axis=2)
        for d in (_dev(ctx, img), _offset_view(ctx, img, 11)):
            assert np.array_equal(_get(f.LUT(d, one)), one[img]) and np.array_equal(_get(f.LUT(d, one.reshape(1, 256))), one[img])
            if cn > 1:
                assert np.array_equal(_get(f.LUT(d, per)), exp_per) and np.array_equal(_get(f.LUT(d, per.reshape(1, 256, cn))), exp_per)
    g = rng.integers(0, 256, (4, 9), dtype=np.uint8)
    assert np.array_equal(_get(f.LUT(_dev(ctx, g), one)), one[g])


@pytest.mark.parametrize("cn", [2, 3, 4])
def test_split_merge_extract(vp, cn):
    from vision import cv2_facade as f
    ctx = vp.default_context()
    rng = np.random.default_rng(10 + cn)
    shapes = [(3, w, cn) for w in (1, 7, 64, 67)] + ([(1080, 1920, 3)] if cn == 3 else [])
    for shape in shapes:
        x = rng.integers(0, 256, shape, dtype=np.uint8)
        for d in ((_dev(ctx, x),) if x.size > 10000 else (_dev(ctx, x), _offset_view(ctx, x, 5))):
            planes = f.split(d)
            assert len(planes) == cn and all(p.shape == shape[:2] for p in planes)
            assert all(p._buf is planes[0]._buf and (p.dev_ptr - planes[0].dev_ptr) % 256 == 0 for p in planes)
            back = f.merge(planes)
            _resident(d, back, *planes)
            assert back.shape == shape and np.array_equal(back.host_copy(), x)
            for c in range(cn):
                assert np.array_equal(planes[c].host_copy(), x[:, :, c])
                if x.size < 10000 or c == 1:
                    assert np.array_equal(_get(f.extractChannel(d, c)), x[:, :, c])
            # planes mixed between device and numpy, and planes that do not start at a 16-byte boundary
            mixed = [planes[c] if c % 2 == 0 else np.ascontiguousarray(x[:, :, c]) for c in range(cn)]
            assert np.array_equal(_get(f.merge(mixed)), x)
            if x.size < 10000:
                odd = [_offset_view(ctx, np.ascontiguousarray(x[:, :, c]), 1 + c) for c in range(cn)]
                assert np.array_equal(_get(f.merge(odd)), x)
    g = rng.integers(0, 256, (5, 9), dtype=np.uint8)
    dg = _dev(ctx, g)
    (only,) = f.split(dg)
    assert only is not dg and only._buf is not dg._buf and np.array_equal(_get(only), g) and np.array_equal(_get(f.extractChannel(dg, 0)), g)
    assert type(f.merge([g, g])) is np.ndarray


def test_count_non_zero(vp):
    from vision import cv2_facade as f
    ctx = vp.default_context()
    rng = np.random.default_rng(12)
    for n in (1, 63, 64, 65, 4097):
        x = rng.choice(np.array([0, 0, 1, 128, 255], np.uint8), (1, n))
        for d in (_dev(ctx, x), _offset_view(ctx, x, 3), _offset_view(ctx, x, 15)):
            assert f.countNonZero(d) == int(np.count_nonzero(x))
            _resident(d)
        for pos in (0, n - 1):
            one = np.zeros((1, n), np.uint8)
            one[0, pos] = 1
            assert f.countNonZero(_dev(ctx, one)) == 1 and f.countNonZero(_offset_view(ctx, one, 7)) == 1
        assert f.countNonZero(_dev(ctx, np.zeros((1, n), np.uint8))) == 0
    full, half = _dev(ctx, np.full((1080, 1920), 255, np.uint8)), _dev(ctx, np.repeat(np.array([[0, 9]], np.uint8), 500, axis=0))
    assert f.countNonZero(full) == 1080 * 1920
    assert f.countNonZero(half) == 500 and f.countNonZero(full) == 1080 * 1920 and f.countNonZero(half) == 500      # calls do not disturb each other
    assert f.countNonZero(_dev(ctx, np.zeros((1080, 1920), np.uint8))) == 0
    assert f.countNonZero(_dev(ctx, np.ones((4, 5, 1), np.uint8))) == 20


@pytest.mark.parametrize("w,h", [(67, 45), (640, 360)])
def test_preprocessor_bias_stays_on_the_device(vp, oracle, w, h):
    """modules/preprocessor.py:89-114 through the cv2 stand-in on a device image: split -> add(bias, plane) -> merge, twice, then the blur."""
    import sys
    import module_harness as MH
    from vision import cv2_facade
    had = sys.modules.get("cv2")
    cv2_facade.install()
    try:
        ppx = MH.PreprocessorHarness(MH.LegacyModule())
        ppx.set(PPX_r_bias=17, PPX_b_bias=-9, PPX_gaussian_blur=True, PPX_gaussian_blur_kernel=2)
        img = F.s1_buoy(4, w, h)
        img[0, :8, 2] = [0, 1, 237, 238, 239, 254, 255, 128]              # values on both sides of both saturation points
        img[0, :8, 0] = [0, 8, 9, 10, 255, 254, 1, 128]
        d = _dev(vp.default_context(), img)
        (out,) = ppx.process(d)
        _resident(d, out)
        e = img.copy()
        e[:, :, 2] = _sat(e[:, :, 2].astype(np.float64) + 17.0)
        e[:, :, 0] = _sat(e[:, :, 0].astype(np.float64) - 9.0)
        assert out.shape == img.shape and np.array_equal(out.host_copy(), oracle.gaussian_blur(e, (5, 5)))
    finally:
        if had is None:
            sys.modules.pop("cv2", None)
