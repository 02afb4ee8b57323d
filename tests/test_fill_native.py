"""Filled polygons on host images: libvp vp_fill_polys_u8 (host C, exact integer crossings, coverage bit plane) paints exactly the
pixels of the Python statement `draw_polylines(..., thickness=-1)` (tests/fill_restate.py statement); the cv2 stand-in's fillPoly,
boundingRect, convexHull and the host fill_ratio on top of it.  Host code only: runs without a GPU."""
import numpy as np
import pytest

import fill_restate as R
from vision import _vp
from vision import cv2_facade as cv
from vision.utils import draw as D
from vision.utils import feature as F


def _base(shape, seed=3):
    return np.random.default_rng(seed).integers(0, 255, shape).astype(np.uint8)


def test_entry_is_bound():
    assert {"vp_fill_polys_u8", "vp_fill_polys_dev", "vp_fill_rect_dev", "vp_fill_circle_dev"} <= set(_vp.exported_symbols())


@pytest.mark.parametrize("shape", [(110, 200), (110, 200, 3), (110, 200, 4)], ids=["c1", "c3", "c4"])
def test_native_equals_statement(shape):
    cn = 1 if len(shape) == 2 else shape[2]
    base = _base(shape)
    for name, polys in R.CASES.items():
        a = base.copy()
        assert D._native_fill(a, polys, R.COLORS[cn]), name          # the host form has no crossing limit: the comb too
        assert np.array_equal(a, R.expected(base, name, R.COLORS[cn])), (name, shape)
    # all cases in one call: the union
    a = base.copy()
    assert D._native_fill(a, [p for polys in R.CASES.values() for p in polys], R.COLORS[cn])
    want = base.copy()
    for name in R.CASES:
        want[R.coverage(name, 110, 200)] = R.COLORS[cn]
    assert np.array_equal(a, want)


def test_public_entries_take_the_native_path_and_keep_the_pixels():
    base = _base((110, 200, 3))
    for name in ("star", "bowtie", "comb", "blob_with_hole", "one_point"):
        a, b, c = base.copy(), base.copy(), base.copy()
        D.draw_contours(a, R.CASES[name], (7, 200, 255), -1)
        for p in R.CASES[name]:
            D.draw_polylines(b, p, True, (7, 200, 255), -1)
        assert cv.drawContours(c, R.CASES[name], -1, (7, 200, 255), thickness=cv.FILLED) is c
        want = R.expected(base, name, (7, 200, 255))
        assert np.array_equal(a, want) and np.array_equal(b, want) and np.array_equal(c, want), name
    # contourIdx selects one contour
    a = base.copy()
    cv.drawContours(a, R.CASES["blob_with_hole"], 1, (1, 1, 1), -1)
    want = base.copy()
    R.statement(want, R.CASES["blob_with_hole"][1:], np.asarray((1, 1, 1), np.uint8))
    assert np.array_equal(a, want)


def test_strided_view_and_wide_words():
    """A 310-pixel-wide view with a row stride: five 64-bit words of the coverage plane, the last one partial; nothing outside it."""
    big = np.zeros((40, 400, 3), np.uint8)
    view = big[4:36, 20:330]
    ref = np.zeros((32, 310, 3), np.uint8)
    polys = [np.array([[-20, -5], [330, 10], [300, 40], [5, 25]], np.int32), R._star(150, 16, 15, 6, 7), np.array([[309, 0], [309, 31], [250, 31]], np.int32),
             np.array([[60, 3], [70, 3], [70, 29], [60, 29]], np.int32)]
    assert D._native_fill(view, polys, (1, 2, 3))
    R.statement(ref, polys, np.asarray((1, 2, 3), np.uint8))
    assert np.array_equal(view, ref)
    assert ref[5:25, 64:66].all() and ref[10, 255:257].all()                      # (spans do cross word boundaries)
    assert not big[:4].any() and not big[36:].any() and not big[:, :20].any() and not big[:, 330:].any()


def test_python_statement_is_the_fallback():
    """Coordinates beyond +-32767 are refused by the native form (nothing painted) and drawn by the Python loop; so are images it
    cannot take (here: not uint8)."""
    far = [np.array([[10, 10], [40000, 30], [10, 50]], np.int32)]
    a = np.zeros((64, 64), np.uint8)
    assert not D._native_fill(a, far, 255) and not a.any()
    D.draw_contours(a, far, 255, -1)
    want = np.zeros((64, 64), np.uint8)
    R.statement(want, far, np.uint8(255))
    assert np.array_equal(a, want) and a[30, 20] == 255
    f = np.zeros((64, 64), np.float32)
    D.draw_contours(f, R.CASES["triangle"], (2.5,), -1)
    assert f[30, 40] == 2.5
    L = _vp.lib()
    pts, cnt, col = np.array([[1, 1], [5, 1], [3, 4]], np.int32), np.array([3], np.int32), np.zeros(4, np.uint8)
    img = np.zeros((8, 8), np.uint8)
    assert L.vp_fill_polys_u8(img.ctypes.data, 8, 8, 8, 1, pts.ctypes.data, cnt.ctypes.data, 1, col.ctypes.data) == _vp.OK
    assert L.vp_fill_polys_u8(None, 8, 8, 8, 1, pts.ctypes.data, cnt.ctypes.data, 1, col.ctypes.data) == _vp.ERR_INVALID
    assert L.vp_fill_polys_u8(img.ctypes.data, 7, 8, 8, 1, pts.ctypes.data, cnt.ctypes.data, 1, col.ctypes.data) == _vp.ERR_INVALID
    assert L.vp_fill_polys_u8(img.ctypes.data, 8, 8, 8, 5, pts.ctypes.data, cnt.ctypes.data, 1, col.ctypes.data) == _vp.ERR_INVALID
    assert L.vp_strerror(_vp.ERR_CAPACITY) == b"capacity exceeded" and (_vp.ERR_UNSUPPORTED, _vp.ERR_CAPACITY) == (-4, -5)


def test_fill_poly_and_fill_convex_poly():
    base = _base((110, 200, 3), 5)
    polys = R.CASES["triangle"] + R.CASES["star"] + R.CASES["partly_right_bottom"]
    a, want = base.copy(), base.copy()
    assert cv.fillPoly(a, polys, (9, 8, 7)) is a
    R.fill_poly_restate(want, polys, np.asarray((9, 8, 7), np.uint8))
    assert np.array_equal(a, want)
    m, want = np.zeros((110, 200), np.uint8), np.zeros((110, 200), np.uint8)
    cv.fillConvexPoly(m, R.CASES["flat_top_bottom"][0], 255)
    R.statement(want, R.CASES["flat_top_bottom"], np.uint8(255))
    assert np.array_equal(m, want) and m[50, 80] == 255


def test_fill_poly_of_overlapping_polygons_is_the_union():
    """Where two polygons of one call overlap, this stand-in paints the overlap (each polygon filled on its own); cv2's joint even-odd
    rule would leave it unpainted.  Pinned here so that the documented difference cannot change unnoticed."""
    a = np.array([[10, 10], [90, 10], [90, 70], [10, 70]], np.int32)
    b = np.array([[50, 40], [150, 40], [150, 100], [50, 100]], np.int32)
    m = np.zeros((110, 200), np.uint8)
    cv.fillPoly(m, [a, b], 255)
    want = np.zeros((110, 200), np.uint8)
    want[10:71, 10:91] = 255
    want[40:101, 50:151] = 255
    assert np.array_equal(m, want)
    assert m[55, 70] == 255                                     # inside both: painted (cv2: 0)
    joint = np.zeros((110, 200), np.uint8)                      # what one even-odd scanline over both polygons' edges would leave there
    joint[10:71, 10:91] ^= 255
    joint[40:101, 50:151] ^= 255
    assert joint[55, 70] == 0 and int((m != joint).sum()) > 0
    both = np.zeros((110, 200), np.uint8)
    R.fill_poly_restate(both, [a, b], np.uint8(255))
    assert np.array_equal(both, want)


def test_bounding_rect_and_convex_hull():
    c = R.CASES["blob_with_hole"][0]
    assert cv.boundingRect(c) == (20, 20, 66, 57)
    assert cv.boundingRect(np.array([[[3, 4]]], np.int32)) == (3, 4, 1, 1)
    star = R.CASES["star"][0]
    hull = cv.convexHull(star.reshape(-1, 1, 2))
    assert hull.shape[1:] == (1, 2) and hull.dtype == star.dtype
    assert {tuple(p) for p in hull.reshape(-1, 2).tolist()} == {tuple(p) for p in star[0::2].tolist()}            # the five tips
    sq = np.array([[0, 0], [5, 0], [10, 0], [10, 10], [5, 5], [0, 10]], np.int32)                                   # a collinear point and an inner one
    assert {tuple(p) for p in cv.convexHull(sq).reshape(-1, 2).tolist()} == {(0, 0), (10, 0), (10, 10), (0, 10)}
    assert cv.contourArea(cv.convexHull(sq)) == 100.0
    with pytest.raises(cv.error):
        cv.convexHull(sq, returnPoints=False)


def test_host_fill_ratio_is_the_reference_lines():
    """vision_common.py:282-288 statement by statement, the fill being the Python statement."""
    rng = np.random.default_rng(8)
    mat = np.zeros((110, 200, 3), np.uint8)
    threshed = np.where(rng.random((110, 200)) < 0.6, 255, 0).astype(np.uint8)
    gray = rng.integers(0, 255, (110, 200)).astype(np.uint8)
    for name in ("star", "blob_with_hole", "partly_left_top", "triangle"):
        contour = np.asarray(R.CASES[name][0]).reshape(-1, 1, 2)
        for t in (threshed, gray):
            fill_mask = np.zeros(mat.shape[:2], dtype=np.uint8)
            R.statement(fill_mask, [contour], np.uint8(255))
            fill_masked = np.where(fill_mask != 0, t, np.uint8(0))
            want = np.sum(fill_masked) / 255 / cv.contourArea(cv.convexHull(contour))
            got = F.fill_ratio(mat, contour, t)
            assert got == want and 0 < got, name
    assert F.is_clipping(mat, R.CASES["partly_left_top"][0]) and not F.is_clipping(mat, R.CASES["triangle"][0])
    assert F.is_clipping(mat, np.array([[50, 50], [194, 60], [60, 70]], np.int32)) and not F.is_clipping(mat, np.array([[50, 50], [193, 60], [60, 70]], np.int32))
    assert F.contour_center(np.array([[[2, 2]], [[2, 6]], [[6, 6]], [[6, 2]]], np.int32)) == (4.0, 4.0)
    with pytest.raises(ZeroDivisionError):
        F.contour_center(np.array([[[3, 3]]], np.int32))
