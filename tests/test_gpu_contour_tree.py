"""GPU: cv2.findContours RETR_CCOMP / RETR_TREE through the vp_find_contours_tree_* entries - contours, order, hole flags and
hierarchy bit for bit as the statements of contour_tree_restate.py give them (statement (a), the raster scan, where Python can afford
it; statement (b), equal to (a) on every CPU test mask, on full frames), with both forms of the bookkeeping."""
import ctypes as C

import numpy as np
import pytest

import contour_tree_restate as R
import frames as F
from test_contour_tree_statement import concentric, known_shapes, thin_wall_mask

pytestmark = pytest.mark.gpu
MODES = (R.RETR_CCOMP, R.RETR_TREE)


@pytest.fixture(autouse=True, params=["one_block", "launches"])
def bookkeeping_form(request, monkeypatch):
    monkeypatch.setenv("VP_CT_MANY", "0" if request.param == "one_block" else "1")


def _expect(oracle, m, mode, method, statement=R.raster_scan):
    lst = oracle.find_contours(m, 1, method)
    return R.expected(m, mode, list(lst), statement)


def _check(got, exp):
    (gc, gh, gy), (ec, eh, ey) = got, exp
    assert len(gc) == len(ec)
    assert all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(gc, ec))
    assert np.array_equal(np.asarray(gh), eh)
    if len(ec):
        assert gy is not None and gy.dtype == np.int32 and gy.shape == (1, len(ec), 4)
        assert np.array_equal(gy[0], ey)
    else:
        assert gy is None


def _feature(m, mode, method):
    from vision.utils import feature
    return feature.find_contours(m, mode, method, with_holes=True, with_hierarchy=True)


def _entry(vp, name, m, mode, method, max_c, max_p):
    """one direct call of a tree entry: (rc, n_contours, n_points, contours, holes, hierarchy)"""
    from vision.devmat import DeviceMat
    ctx = vp.default_context()
    h, w = m.shape
    pts = np.full((max(max_p, 1), 2), -7, np.int32)
    counts = np.full(max(max_c, 1), -7, np.int32)
    holes = np.full(max(max_c, 1), 7, np.uint8)
    hier = np.full((max(max_c, 1), 4), -7, np.int32)
    nc, npts = C.c_int32(0), C.c_int64(0)
    args = (int(mode), int(method), vp.ptr(pts), max_p, vp.ptr(counts), vp.ptr(holes), max_c, C.byref(nc), C.byref(npts), vp.ptr(hier))
    if name == "u8":
        vp.check(vp.lib().vp_find_contours_tree_u8(ctx.handle, vp.ptr(m), w, w, h, *args), ctx.handle)
    else:
        d = DeviceMat.from_host(ctx, np.ascontiguousarray(m), binary=True)
        vp.check(vp.lib().vp_find_contours_tree_dev(ctx.handle, d.dev_ptr, w, w, h, *args), ctx.handle)
    k, p = nc.value, npts.value
    cs, o = [], 0
    if k <= max_c and p <= max_p:
        for c in counts[:k].tolist():
            cs.append(pts[o:o + c].reshape(-1, 1, 2))
            o += c
    return k, p, cs, holes[:k], hier, counts


@pytest.mark.parametrize("name", sorted(known_shapes()))
def test_known_shapes_every_entry(vp, oracle, name):
    from vision.devmat import DeviceMat
    m = known_shapes()[name]
    ctx = vp.default_context()
    for mode in MODES:
        for method in (1, 2):
            exp = _expect(oracle, m, mode, method)
            _check(_feature(m, mode, method), exp)
            _check(_feature(DeviceMat.from_host(ctx, m, binary=True), mode, method), exp)


def test_random_and_thin_wall_masks(vp, oracle):
    rng = np.random.default_rng(31)
    for trial in range(60):
        h, w = int(rng.integers(1, 40)), int(rng.integers(1, 90))
        m = F.random_mask(rng, h, w) if trial % 3 else thin_wall_mask(rng, h, w)
        for mode in MODES:
            _check(_feature(m, mode, 1 + trial % 2), _expect(oracle, m, mode, 1 + trial % 2))


def test_bit_plane_entry(vp, oracle):
    """a threshold mask that carries its bit plane (w % 64 == 0) goes through vp_find_contours_tree_bits_dev"""
    from vision.devmat import DeviceMat
    from vision.utils import color
    ctx = vp.default_context()
    rng = np.random.default_rng(5)
    gray = (rng.random((96, 256)) * 255).astype(np.uint8)
    gray[10:80, 20:200] = 255
    gray[20:70, 40:180] = 0
    gray[30:60, 60:100] = 255
    th = color.range_threshold(DeviceMat.from_host(ctx, gray), 128, 255)
    assert th._bits is not None
    m = np.asarray(oracle.inrange(gray, 128, 255))
    for mode in MODES:
        for method in (1, 2):
            th = color.range_threshold(DeviceMat.from_host(ctx, gray), 128, 255)
            _check(_feature(th, mode, method), _expect(oracle, m, mode, method))


def test_direct_entries_short_capacities_and_flat_modes(vp, oracle):
    """true totals and nothing copied when a capacity is short; modes 0 / 1 through the tree entries = the old entries, with the
    flat rows [next, prev, -1, -1]"""
    from vision.utils import feature
    m = known_shapes()["two_islands_in_one_hole"]
    for name in ("u8", "dev"):
        for mode in MODES:
            exp = _expect(oracle, m, mode, 2)
            k, p, cs, holes, hier, counts = _entry(vp, name, m, mode, 2, 1, 4096)
            assert k == len(exp[0]) and counts[0] == -7 and hier[0, 0] == -7
            k, p, cs, holes, hier, counts = _entry(vp, name, m, mode, 2, 64, 3)
            assert k == len(exp[0]) and p == sum(len(c) for c in exp[0]) and counts[0] == -7
            k, p, cs, holes, hier, counts = _entry(vp, name, m, mode, 2, 64, 4096)
            _check((cs, holes, hier[:k][None]), exp)
        for mode in (0, 1):
            old, oh = feature.find_contours(m, mode, 2, with_holes=True)
            k, p, cs, holes, hier, counts = _entry(vp, name, m, mode, 2, 64, 4096)
            assert len(cs) == len(old) and all(np.array_equal(a, b) for a, b in zip(cs, old)) and np.array_equal(holes, oh)
            flat = [[j + 1 if j + 1 < k else -1, j - 1, -1, -1] for j in range(k)]
            assert hier[:k].tolist() == flat
            got = feature.find_contours(m, mode, 2, with_hierarchy=True)
            assert got[1][0].tolist() == flat


def test_full_frames(vp, oracle):
    """S1 / S2 1080p threshold masks, 2 % and 10 % speckle (17 k / 143 k contours: above the wrapper's first capacities), a 4K
    frame, and concentric rings 540 deep"""
    from vision.utils import color
    rng = np.random.default_rng(11)
    masks = [oracle.inrange(oracle.bgr2lab(F.s1_buoy(0))[:, :, 1].copy(), 150, 255),
             oracle.inrange(oracle.bgr2hsv(F.s2_bins(0)), (10, 20, 60), (30, 100, 255)),
             F.random_mask(rng, 1080, 1920, 0.02), F.random_mask(rng, 1080, 1920, 0.10),
             concentric(1080, 1920)]
    yy, xx = np.mgrid[0:2160, 0:3840]
    m4 = np.zeros((2160, 3840), np.uint8)
    for _ in range(30):
        cx, cy, r = rng.uniform(0, 3840), rng.uniform(0, 2160), rng.uniform(10, 400)
        m4[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 255
    for _ in range(30):
        cx, cy, r = rng.uniform(0, 3840), rng.uniform(0, 2160), rng.uniform(5, 150)
        m4[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 0
    masks.append(m4)
    for i, m in enumerate(masks):
        m = np.ascontiguousarray(m)
        for mode in MODES:
            got = _feature(m, mode, 2)
            _check(got, _expect(oracle, m, mode, 2, R.topological))
            if i == 4 and mode == R.RETR_TREE:
                assert int(got[2][0][-1][3]) == len(got[0]) - 2          # one chain: every border the child of the one before it
                assert len(got[0]) >= 500
        if i == 3:
            assert len(got[0]) > 100000


def test_facade_tree_on_a_module_mask(vp, oracle):
    from vision import cv2_facade as cv2
    img = F.s2_bins(0, 320, 180)
    mask = oracle.morph(oracle.OPEN, oracle.inrange(oracle.bgr2hsv(img), (10, 20, 60), (30, 100, 255)),
                        np.ones((5, 5), np.uint8))
    mask = np.ascontiguousarray(mask)
    for mode in MODES:
        cs, hier = cv2.findContours(mask, mode, cv2.CHAIN_APPROX_SIMPLE)
        exp = _expect(oracle, mask, mode, 2)
        _check((cs, exp[1], hier), exp)
    assert cv2.findContours(np.zeros((8, 8), np.uint8), cv2.RETR_TREE, cv2.CHAIN_APPROX_SIMPLE) == ((), None)
