"""Filled polygons, rectangles and discs written by the device into images that live there (libvp vp_fill_polys_dev,
vp_fill_rect_dev, vp_fill_circle_dev; kernels in csrc/vp_fill.hip): the pixels of the Python statement (tests/fill_restate.py), and
the image never visits the host."""
import numpy as np
import pytest

import fill_restate as R

pytestmark = pytest.mark.gpu


def _base(shape, seed=3):
    return np.random.default_rng(seed).integers(0, 255, shape).astype(np.uint8)


def _shape(w, cn):
    return (110, w) if cn == 1 else (110, w, cn)


@pytest.mark.parametrize("cn", [1, 3, 4])
@pytest.mark.parametrize("w", [64, 65, 200])
def test_draw_contours_filled_stays_on_the_device(vp, w, cn):
    from vision.devmat import DeviceMat
    from vision.utils import draw as D
    ctx = vp.default_context()
    base = _base(_shape(w, cn))
    for name, polys in R.CASES.items():
        dev = DeviceMat.from_host(ctx, base)
        D.draw_contours(dev, polys, R.COLORS[cn], -1)
        if name in R.DEVICE_REFUSES:
            assert dev._host is not None, name                   # the Python layer fell back to the host
        else:
            assert dev._host is None, f"{name}: the fill downloaded the image"
        assert np.array_equal(dev.host_copy(), R.expected(base, name, R.COLORS[cn])), (name, w, cn)


def test_polylines_entry_and_an_unaligned_image(vp):
    """draw_polylines(thickness=-1) takes the same path; a plane at an odd byte offset inside its allocation (spans start at any
    alignment, the 16-byte stores must not)."""
    from vision.devmat import DeviceMat, _DevBuf
    from vision.utils import draw as D
    ctx = vp.default_context()
    base = _base((110, 200, 3))
    dev = DeviceMat.from_host(ctx, base)
    D.draw_polylines(dev, R.CASES["star"][0], True, (7, 200, 255), -1)
    assert dev._host is None and np.array_equal(dev.host_copy(), R.expected(base, "star", (7, 200, 255)))
    for off, shape in ((1, (110, 200)), (7, (110, 65, 3)), (13, (110, 64, 4))):
        cn = 1 if len(shape) == 2 else shape[2]
        b = _base(shape, off)
        buf = _DevBuf(ctx, b.nbytes + 64)
        m = DeviceMat.over_buffer(ctx, buf, off, shape, np.uint8)
        vp.check(vp.lib().vp_memcpy_h2d(ctx.handle, m.dev_ptr, b.ctypes.data, b.nbytes), ctx.handle)
        for name in ("star", "covers_everything", "blob_with_hole"):
            vp.check(vp.lib().vp_memcpy_h2d(ctx.handle, m.dev_ptr, b.ctypes.data, b.nbytes), ctx.handle)
            assert D._device_fill(m, R.CASES[name], R.COLORS[cn])
            assert np.array_equal(m.host_copy(), R.expected(b, name, R.COLORS[cn])), (name, off)


def test_forty_polygons_in_one_call(vp):
    from vision.devmat import DeviceMat
    from vision.utils import draw as D
    ctx = vp.default_context()
    rng = np.random.default_rng(40)
    polys = [(rng.integers(-8, 9, (int(rng.integers(3, 8)), 2)) + rng.integers(0, (200, 110), 2)).astype(np.int32) for _ in range(40)]
    base = _base((110, 200, 3))
    dev = DeviceMat.from_host(ctx, base)
    D.draw_contours(dev, polys, (7, 200, 255), -1)
    want = base.copy()
    R.statement(want, polys, np.asarray((7, 200, 255), np.uint8))
    assert dev._host is None and np.array_equal(dev.host_copy(), want)
    # sixteen triangles: few enough points for the argument form of the outline, too many polygons for that of the fill
    tris = polys[:16]
    tris = [p[:3] for p in tris]
    dev = DeviceMat.from_host(ctx, base)
    D.draw_contours(dev, tris, (7, 200, 255), -1)
    want = base.copy()
    R.statement(want, tris, np.asarray((7, 200, 255), np.uint8))
    assert dev._host is None and np.array_equal(dev.host_copy(), want)


def test_comb_is_refused_whole_and_falls_back(vp):
    from vision.devmat import DeviceMat
    from vision.utils import draw as D
    ctx = vp.default_context()
    base = _base((110, 200))
    dev = DeviceMat.from_host(ctx, base)
    # a polygon the kernel can fill in front of the comb: the call must not paint it either
    assert D._device_fill(dev, R.CASES["triangle"] + R.CASES["comb"], 180) is False
    assert dev._host is None and np.array_equal(dev.host_copy(), base)
    pts = np.ascontiguousarray(R.CASES["comb"][0], np.int32)
    cnt, col = np.array([len(pts)], np.int32), np.full(4, 180, np.uint8)
    assert vp.lib().vp_fill_polys_dev(ctx.handle, dev.dev_ptr, 200, 110, 1, pts.ctypes.data, cnt.ctypes.data, 1, col.ctypes.data) == vp.ERR_CAPACITY
    far = np.array([[10, 10], [40000, 30], [10, 50]], np.int32)
    cnt = np.array([3], np.int32)
    assert vp.lib().vp_fill_polys_dev(ctx.handle, dev.dev_ptr, 200, 110, 1, far.ctypes.data, cnt.ctypes.data, 1, col.ctypes.data) == vp.ERR_UNSUPPORTED
    assert vp.lib().vp_fill_polys_dev(ctx.handle, None, 200, 110, 1, far.ctypes.data, cnt.ctypes.data, 1, col.ctypes.data) == vp.ERR_INVALID
    assert np.array_equal(dev.host_copy(), base)
    D.draw_contours(dev, R.CASES["comb"], 180, -1)
    assert np.array_equal(dev.host_copy(), R.expected(base, "comb", 180))


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_filled_rect_and_disc(vp, cn):
    from vision.devmat import DeviceMat
    from vision.utils import draw as D
    ctx = vp.default_context()
    for w in (64, 65, 200):
        base = _base(_shape(w, cn), w)
        color = R.COLORS[cn]
        for r in (0, 1, 7, 50):
            for c in ((30, 40), (0, 0), (w - 1, 109), (w // 2, 0), (-5, 50), (w + 20, 120), (20, -60), (-100, -100)):
                dev, want = DeviceMat.from_host(ctx, base), base.copy()
                D.draw_circle(dev, c, r, color, -1)
                D.draw_circle(want, c, r, color, -1)
                assert dev._host is None and np.array_equal(dev.host_copy(), want), (w, cn, r, c)
        for p1, p2 in (((10, 20), (50, 70)), ((50, 70), (10, 20)), ((-10, -10), (w + 10, 200)), ((5, 5), (5, 5)), ((w - 1, 0), (w - 1, 109)), ((-30, 10), (-5, 40)),
                       ((3, 90), (w - 4, 300)), ((0, 0), (15, 0))):
            dev, want = DeviceMat.from_host(ctx, base), base.copy()
            D.draw_rect(dev, p1, p2, color, -1)
            D.draw_rect(want, p1, p2, color, -1)
            assert dev._host is None and np.array_equal(dev.host_copy(), want), (w, cn, p1, p2)


def test_binary_flag_follows_the_colour(vp):
    from vision.devmat import DeviceMat
    from vision.utils import draw as D
    ctx = vp.default_context()
    mask = np.zeros((110, 200), np.uint8)
    for color, keeps in ((255, True), (0, True), (180, False)):
        dev = DeviceMat.from_host(ctx, mask, binary=True)
        D.draw_contours(dev, R.CASES["star"], color, -1)
        assert dev.binary is keeps
        dev = DeviceMat.from_host(ctx, mask, binary=True)
        D.draw_circle(dev, (50, 50), 9, color, -1)
        assert dev.binary is keeps
    dev = DeviceMat.from_host(ctx, mask)                          # not known to be a mask: stays unknown
    D.draw_contours(dev, R.CASES["star"], 255, -1)
    assert dev.binary is False


def test_fill_ratio_on_device_images(vp):
    from vision.devmat import DeviceMat
    from vision.utils import feature as F
    ctx = vp.default_context()
    rng = np.random.default_rng(8)
    mat = np.zeros((110, 200, 3), np.uint8)
    threshed = np.where(rng.random((110, 200)) < 0.6, 255, 0).astype(np.uint8)
    gray = rng.integers(0, 255, (110, 200)).astype(np.uint8)
    for name in ("star", "blob_with_hole", "partly_left_top", "comb"):
        contour = np.asarray(R.CASES[name][0]).reshape(-1, 1, 2)
        for host, binary in ((threshed, True), (gray, False)):
            dev = DeviceMat.from_host(ctx, host, binary=binary)
            got = F.fill_ratio(DeviceMat.from_host(ctx, mat), contour, dev)
            assert got == F.fill_ratio(mat, contour, host) and got > 0, (name, binary)
            assert dev._host is None


def test_deferred_result_is_computed_before_the_fill(vp):
    """An operator result that has not been launched yet reads its input as it was when the operator was called, also when a fill
    changes that input afterwards; and a deferred result used as the target is computed, then filled."""
    from vision import cv2_facade as cv
    from vision.devmat import DeviceMat, defer_enabled
    from vision.utils import draw as D
    ctx = vp.default_context()
    a = np.where(_base((110, 200), 21) > 128, 255, 0).astype(np.uint8)
    da = DeviceMat.from_host(ctx, a, binary=True)
    inv = cv.bitwise_not(da)
    assert not defer_enabled() or inv._pending is not None
    D.draw_contours(da, R.CASES["star"], 255, -1)                 # the input changes: the pending operator runs first
    assert np.array_equal(inv.host_copy(), ~a)
    assert np.array_equal(da.host_copy(), R.expected(a, "star", 255))
    inv2 = cv.bitwise_not(DeviceMat.from_host(ctx, a, binary=True))
    D.draw_contours(inv2, R.CASES["bowtie"], 0, -1)               # the target itself is pending
    assert inv2._host is None and np.array_equal(inv2.host_copy(), R.expected(~a, "bowtie", 0))


@pytest.mark.parametrize("color", [255, 0])
def test_pending_mask_with_a_bit_plane_as_the_target(vp, color):
    """A 0/255 mask that is still a pending operator result and whose width is a multiple of 64 gets its bit plane from its own launch.
    Filled (or outlined) in place with 0 or 255 it must not keep that plane: contours, the count and the labelling that follow see the
    painted mask."""
    from vision import cv2_facade as cv
    from vision.devmat import DeviceMat, defer_enabled
    from vision.utils import draw as D
    from vision.utils import feature as F
    ctx = vp.default_context()
    yy, xx = np.mgrid[:110, :128]
    a = np.where(((xx // 16 + yy // 16) % 2 == 0) & (xx > 8) & (yy > 8), 255, 0).astype(np.uint8)      # a checkerboard of blobs
    polys = [np.array([[20, 15], [110, 30], [70, 100]], np.int32)]
    cov = np.zeros((110, 128), np.uint8)
    R.statement(cov, polys, np.uint8(1))
    outline = np.zeros((110, 128), np.uint8)
    D.draw_contours(outline, polys, 1, 1)

    def pending():
        m = cv.bitwise_not(DeviceMat.from_host(ctx, a, binary=True))
        assert not defer_enabled() or m._pending is not None
        return m

    def same_contours(got, want):
        return len(got) == len(want) and all(np.array_equal(x, y) for x, y in zip(got, want))
    for paint, covered in ((lambda m: D.draw_contours(m, polys, color, -1), cov), (lambda m: D.draw_circle(m, (64, 55), 30, color, -1), None),
                           (lambda m: D.draw_contours(m, polys, color, 1), outline)):
        m = pending()
        paint(m)
        if covered is None:
            want = ~a
            D.draw_circle(want, (64, 55), 30, color, -1)
        else:
            want = np.where(covered != 0, np.uint8(color), ~a)
        assert m._host is None
        assert same_contours(F.outer_contours(m), F.outer_contours(want))
        assert cv.countNonZero(m) == int(np.count_nonzero(want))
        n_dev, n_host = cv.connectedComponentsWithStats(m)[0], cv.connectedComponentsWithStats(want)[0]
        assert n_dev == n_host
        assert np.array_equal(m.host_copy(), want)


def test_1080p_disc_contour_equals_the_native_host_form(vp):
    from vision.devmat import DeviceMat
    from vision.utils import draw as D
    from vision.utils import feature as F
    ctx = vp.default_context()
    yy, xx = np.mgrid[:1080, :1920]
    disc = np.where((xx - 960) ** 2 + (yy - 540) ** 2 <= 400 ** 2, 255, 0).astype(np.uint8)
    contours = F.outer_contours(disc)
    assert len(contours) == 1 and len(contours[0]) > 500
    base = _base((1080, 1920, 3))
    want = base.copy()
    assert D._native_fill(want, contours, (7, 200, 255))
    dev = DeviceMat.from_host(ctx, base)
    D.draw_contours(dev, contours, (7, 200, 255), -1)
    assert dev._host is None and np.array_equal(dev.host_copy(), want)
    assert np.array_equal((want == np.asarray((7, 200, 255), np.uint8)).all(2) | (disc == 0), np.ones((1080, 1920), bool))   # the disc is covered
