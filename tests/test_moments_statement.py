"""CPU suite for the statement of cv2.moments / cv2.HuMoments (tests/moments_restate.py): it is checked against witnesses that share
no code with it - a float-free brute force, the closed forms of a rectangle, and the invariances the moments are named for, on shapes
small enough that every double operation is exact - and the two host-only entries of libvp.so (vp_polygon_moments,
vp_moments_complete) and the Python Hu arithmetic of the library equal it bit for bit."""
import ctypes as C
from fractions import Fraction

import numpy as np

import moments_restate as R


def _lib():
    from vision import _vp
    lib = C.CDLL(_vp.LIB_PATH)
    for name in ("vp_polygon_moments", "vp_moments_complete"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _vp._SIGS[name]
    return lib


def _brute(img, binary):
    out = [0] * 10
    for y in range(img.shape[0]):
        for x in range(img.shape[1]):
            v = int(img[y, x])
            if binary:
                v = 1 if v else 0
            for k, (p, q) in enumerate(R.ORDER):
                out[k] += x ** p * y ** q * v
    return tuple(out)


def test_raster_sums_equal_a_float_free_brute_force():
    rng = np.random.default_rng(11)
    for h, w in ((1, 1), (1, 9), (9, 1), (2, 2), (5, 7), (13, 4)):
        for img in (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.choice(np.array([0, 3, 255], np.uint8), (h, w)), np.zeros((h, w), np.uint8),
                    np.full((h, w), 255, np.uint8)):
            for binary in (False, True):
                got = R.raster_moments(img, binary)
                assert all(type(v) is int for v in got) and got == _brute(img, binary), (h, w, binary)


def test_raster_sums_do_not_wrap_where_int64_would():
    """all-255 at 2 x 2100: x^3 passes 2^32 and the sums are Python ints whichever path added the rows"""
    img = np.full((2, 2100), 255, np.uint8)
    t = 2099 * 2100 // 2
    got = R.raster_moments(img)
    assert got[0] == 255 * 2 * 2100 and got[6] == 255 * 2 * t * t and got[9] == 255 * 2100 * 1
    assert R.raster_moments(np.ascontiguousarray(img.T))[9] == got[6]


def test_label_sums_equal_the_raster_sums_of_each_label_and_skip_what_is_out_of_range():
    rng = np.random.default_rng(5)
    labels = rng.integers(-1, 5, (9, 11)).astype(np.int32)              # -1 and 4 are out of range for nlabels = 4
    got = R.label_moments(labels, 4)
    assert len(got) == 4
    for k in range(4):
        assert got[k] == R.raster_moments((labels == k).astype(np.uint8), True), k
    assert sum(r[0] for r in got) == int(((labels >= 0) & (labels < 4)).sum())


def test_contour_moments_of_a_rectangle_equal_the_closed_forms():
    """the polygon (x0, y0) .. (x1, y1): m_pq = (x1^(p+1) - x0^(p+1)) / (p + 1) * (y1^(q+1) - y0^(q+1)) / (q + 1).  With these small
    integer corners every sum of the loop is an exact integer; what is rounded is the factor 1/6 .. 1/60 and the one product with it,
    half an ulp each: 2^-51 relative covers both."""
    for x0, y0, x1, y1 in ((0, 0, 4, 3), (2, 5, 9, 11), (10, 1, 13, 40)):
        for pts in ([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], [(x0, y0), (x0, y1), (x1, y1), (x1, y0)]):       # both orientations
            for dtype in (np.int32, np.float32):
                got = R.contour_moments(np.array(pts, dtype).reshape(-1, 1, 2))
                for k, (p, q) in enumerate(R.ORDER):
                    exp = Fraction(x1 ** (p + 1) - x0 ** (p + 1), p + 1) * Fraction(y1 ** (q + 1) - y0 ** (q + 1), q + 1)
                    assert abs(Fraction(got[k]) - exp) <= exp * Fraction(1, 2 ** 51), (pts, k, got[k], float(exp))


def _shape16():
    """16 pixels without any symmetry: m00 is a power of two, so 1 / m00, the centre and every product below are exact in float64"""
    s = np.zeros((6, 7), np.uint8)
    s[0, 0:5] = 1
    s[1, 0:4] = 1
    s[2, 1:4] = 1
    s[3, 2:4] = 1
    s[4, 3] = 1
    s[5, 3] = 1
    assert int(s.sum()) == 16
    return s


def test_central_moments_do_not_move_with_the_shape():
    s = _shape16()
    base = R.complete(R.raster_moments(s))
    for dy, dx in ((0, 1), (3, 0), (17, 40), (250, 3)):
        canvas = np.zeros((s.shape[0] + dy, s.shape[1] + dx), np.uint8)
        canvas[dy:, dx:] = s
        moved = R.complete(R.raster_moments(canvas))
        assert moved[0] == base[0] and (moved[1] != base[1]) == (dx != 0) and (moved[2] != base[2]) == (dy != 0)
        assert R.as_bytes(moved[10:]) == R.as_bytes(base[10:]), (dy, dx)


def test_hu_invariants_survive_a_quarter_turn_exactly():
    """four pixels: the centre is a multiple of 1/4, the mu a multiple of 1/16, sqrt(1 / m00) = 1/2 - every operation of `hu` is exact,
    so the seven numbers of the turned shape are the same doubles"""
    s = np.zeros((2, 3), np.uint8)
    s[0, :] = 1
    s[1, 0] = 1
    base = R.hu(R.complete(R.raster_moments(s)))
    assert base[0] > 0 and any(v != 0 for v in base[1:])
    t = s
    for _ in range(3):
        t = np.ascontiguousarray(np.rot90(t))
        assert R.as_bytes(R.hu(R.complete(R.raster_moments(t)))) == R.as_bytes(base)
    mirrored = R.hu(R.complete(R.raster_moments(np.ascontiguousarray(s[:, ::-1]))))
    assert R.as_bytes(mirrored[:6]) == R.as_bytes(base[:6]) and mirrored[6] == -base[6] != 0      # the seventh tells a reflection


def _contours():
    rng = np.random.default_rng(23)
    for n in (3, 4, 7, 64, 500):
        yield rng.integers(0, 32768, (n, 1, 2)).astype(np.int32)
        yield rng.integers(-32767, 32768, (n, 2)).astype(np.int32)
        yield (rng.random((n, 1, 2)) * 2000 - 300).astype(np.float32)
    yield np.zeros((0, 1, 2), np.int32)
    yield np.array([[[5, 7]]], np.int32)                                           # one point
    yield np.array([[[5, 7]], [[9, 2]]], np.int32)                                 # two: no area
    yield np.array([[0, 0], [4, 4], [8, 8], [2, 2]], np.int32)                      # collinear: no area
    yield np.array([[0, 0], [0, 5], [6, 5], [6, 0]], np.int32)                      # one orientation ...
    yield np.array([[0, 0], [6, 0], [6, 5], [0, 5]], np.int32)                      # ... and the other
    yield np.array([[0.25, 0.5], [10.75, 0.5], [3.5, 8.125]], np.float32)
    yield np.array([[0, 0], [1e-5, 0], [0, 1e-5]], np.float32)                      # |a00| below FLT_EPSILON: all zero


def test_library_contour_moments_equal_the_statement_bit_for_bit():
    lib = _lib()
    seen_zero = seen_neg = 0
    for c in _contours():
        pts = np.ascontiguousarray(c.reshape(-1, 2))
        out = np.full(10, 7.0)
        assert lib.vp_polygon_moments(pts.ctypes.data if len(pts) else None, int(pts.dtype == np.float32), len(pts), out.ctypes.data) == 0
        exp = R.contour_moments(c)
        assert out.tobytes() == R.as_bytes(exp), (c.dtype, len(pts), out, exp)
        seen_zero += exp[0] == 0
        a = pts.astype(np.float64)
        seen_neg += len(a) > 2 and float(np.sum(np.roll(a[:, 0], 1) * a[:, 1] - a[:, 0] * np.roll(a[:, 1], 1))) < 0
        assert exp[0] >= 0
    assert seen_zero >= 5 and seen_neg >= 1
    assert lib.vp_polygon_moments(None, 0, 3, np.zeros(10).ctypes.data) != 0 and lib.vp_polygon_moments(None, 0, -1, np.zeros(10).ctypes.data) != 0


def _spatial_rows():
    for c in _contours():
        yield R.contour_moments(c)
    rng = np.random.default_rng(2)
    for h, w in ((1, 1), (5, 7), (40, 33)):
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        yield R.raster_moments(img)
        yield R.raster_moments(img, True)
    yield R.raster_moments(np.zeros((3, 3), np.uint8))                             # m00 = 0
    yield R.raster_moments(np.full((1080, 1920), 255, np.uint8))                    # m30 above 2^53: rounded once
    yield (-4.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0)                       # a negative m00 takes |1 / m00| under the root
    yield (1e-17, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0)                      # below DBL_EPSILON: no centre


def test_library_complete_and_hu_equal_the_statement_bit_for_bit():
    from vision.utils import feature
    lib = _lib()
    n = 0
    for m in _spatial_rows():
        m = np.array([float(v) for v in m], np.float64)
        out = np.full(24, 7.0)
        assert lib.vp_moments_complete(m.ctypes.data, out.ctypes.data) == 0
        exp = R.complete(m)
        assert out.tobytes() == R.as_bytes(exp), (m, out, exp)
        assert feature.hu_moments(out).tobytes() == R.as_bytes(R.hu(exp))
        assert feature.hu_moments(feature.moments_dict(out)).tobytes() == R.as_bytes(R.hu(exp))
        assert feature.orientation(out) == feature.orientation(feature.moments_dict(out))
        n += 1
    assert n > 20
    assert lib.vp_moments_complete(None, np.zeros(24).ctypes.data) != 0


def test_feature_contour_moments_are_the_two_entries_chained():
    from vision.utils import feature
    for c in _contours():
        got = feature.contour_moments(c)
        assert got.dtype == np.float64 and got.shape == (24,)
        assert got.tobytes() == R.as_bytes(R.complete(R.contour_moments(c)))
    square = np.array([[0, 0], [0, 4], [8, 4], [8, 0]], np.int32)
    assert abs(feature.orientation(feature.contour_moments(square))) < 1e-12        # wider than tall: along x
    tall = np.array([[0, 0], [0, 8], [4, 8], [4, 0]], np.int32)
    assert abs(abs(feature.orientation(feature.contour_moments(tall))) - np.pi / 2) < 1e-12
    assert feature._polygon_moments(square) == tuple(feature.contour_moments(square)[:3])
