"""CPU suite for the host half of the contour geometry: vp_min_enclosing_circle_i32 against the brute-force statement
(tests/geometry_restate.py) on small point sets - random, duplicated, collinear, right and obtuse triangles, cocircular points - and on
known answers; min_enclosing_circle and cv2_facade.minEnclosingCircle return values; the factored calipers still give the statement's
rectangle; fitEllipse stays outside.

Tolerance of the circle: centre and radius within 1 float32 ulp of the correctly rounded exact value.  The library computes each from
exact integers with a handful of float64 roundings (relative error about 2^-51), far below half a float32 ulp (2^-24): only when the
exact value lies that close to a float32 rounding boundary can the result move, and then by one ulp."""
import ctypes as C
import math

import numpy as np
import pytest

import geometry_restate as R


def _circle(pts):
    from vision import _vp
    p = np.ascontiguousarray(np.asarray(pts, np.int32).reshape(-1, 2))
    out = (C.c_float * 3)()
    sup = (C.c_int32 * 7)()
    assert _vp.lib().vp_min_enclosing_circle_i32(p.ctypes.data, len(p), out, sup) == 0
    n = sup[0]
    return np.array(out[:], np.float32), [(sup[1 + 2 * k], sup[2 + 2 * k]) for k in range(n)]


def _check(pts):
    got, sup = _circle(pts)
    exact = R.min_enclosing_circle(pts)
    want = R.circle_f32(exact)
    for g, w in zip(got, want):
        assert R.ulps(g, w) <= 1, (pts, got, want)
    if len(pts):
        assert 1 <= len(sup) <= 3 and R.support_circle(sup) == exact, (pts, sup, exact)
        assert R.is_min_circle_of(sup, pts)


def _cases():
    rng = np.random.default_rng(20260521)
    cases = []
    for n in range(1, 13):
        for _ in range(6):
            cases.append(rng.integers(0, 32, (n, 2)).tolist())
    for _ in range(10):                                                       # duplicates
        base = rng.integers(0, 32, (4, 2))
        cases.append(base[rng.integers(0, 4, 11)].tolist())
    cases += [[[i, 3] for i in range(7)], [[2 * i, 5 * i] for i in range(6)], [[5, 5]] * 4, [[i, 31 - i] for i in (9, 0, 31, 4)]]   # collinear
    cases += [[[0, 0], [6, 0], [0, 8]], [[0, 0], [10, 0], [3, 1]], [[0, 0], [10, 0], [5, 5]], [[0, 0], [31, 0], [15, 2], [16, 30]]]   # right, obtuse, on the diameter circle
    cases += [[[0, 0], [4, 0], [4, 4], [0, 4]], [[5, 0], [0, 5], [-5, 0], [0, -5], [3, 4], [-4, 3]], [[1, 7], [7, 1], [1, 1], [7, 7], [4, 4]]]   # cocircular
    return cases


@pytest.mark.parametrize("part", range(4))
def test_host_circle_matches_the_brute_force_statement(part):
    cases = _cases()
    for pts in cases[part::4]:
        _check(pts)


def test_known_answers():
    got, sup = _circle([[0, 0], [4, 0], [4, 4], [0, 4]])
    assert got[0] == 2 and got[1] == 2 and got[2] == np.float32(math.sqrt(8.0))
    got, sup = _circle([[7, -3]])
    assert got.tolist() == [7.0, -3.0, 0.0] and sup == [(7, -3)]
    got, sup = _circle(np.zeros((0, 2), np.int32))
    assert got.tolist() == [0.0, 0.0, 0.0] and sup == []
    got, sup = _circle([[-32768, -32768], [32767, 32767]])
    assert got[0] == np.float32(-0.5) and got[1] == np.float32(-0.5) and R.ulps(got[2], R.round_f32_sqrt(R.Fraction(2 * 65535 ** 2, 4))) <= 1


def test_rounding_helpers_of_the_statement():
    assert R.round_f32(R.Fraction(1, 3)) == np.float32(1 / 3) and R.round_f32(R.Fraction(-5, 2)) == np.float32(-2.5)
    assert R.round_f32((1 << 24) + 1) == np.float32(1 << 24) and R.round_f32((1 << 24) + 3) == np.float32((1 << 24) + 4)   # ties to even
    for q in (2, 8, R.Fraction(1, 2), 10 ** 9 + 7, R.Fraction(12345, 4)):
        assert R.round_f32_sqrt(q) == np.float32(math.sqrt(float(q))), q
    assert R.ulps(np.float32(1), np.nextafter(np.float32(1), np.float32(2))) == 1 and R.ulps(np.float32(-0.0), np.float32(0.0)) == 0


def test_python_entries_return_values():
    """min_enclosing_circle raised NotImplementedError and the facade had no minEnclosingCircle before the geometry pass existed."""
    from vision import cv2_facade
    from vision.utils import feature
    sq = np.array([[[0, 0]], [[4, 0]], [[4, 4]], [[0, 4]]], np.int32)
    (cx, cy), r = feature.min_enclosing_circle(sq)
    assert (cx, cy) == (2.0, 2.0) and r == float(np.float32(math.sqrt(8.0)))
    assert cv2_facade.minEnclosingCircle(sq) == ((cx, cy), r)
    assert cv2_facade.minEnclosingCircle(sq.astype(np.float32)) == ((cx, cy), r)      # integer-valued floats
    assert feature.min_enclosing_circle(np.array([[[9, 9]]], np.int32)) == ((9.0, 9.0), 0.0)
    with pytest.raises(cv2_facade.error):
        cv2_facade.minEnclosingCircle(np.array([[0.5, 0.0], [1.0, 1.0]], np.float32))
    with pytest.raises(ValueError):
        feature.min_enclosing_circle(np.array([[0, 0], [40000, 0]], np.int32))


def test_ellipse_fits_stay_outside():
    from vision import cv2_facade
    from vision.utils import feature
    with pytest.raises(NotImplementedError):
        feature.min_enclosing_ellipse(np.zeros((5, 1, 2), np.int32))
    with pytest.raises((AttributeError, NotImplementedError, cv2_facade.error)):
        cv2_facade.fitEllipse(np.zeros((5, 1, 2), np.int32))


def test_factored_calipers_give_the_statements_rectangle():
    """vp_min_area_rect_i32 after its tail became vp_min_area_rect_finish: still the floats of _min_area_rect_loop, also beyond the
    coordinate bound of the device pass"""
    from vision import _vp
    rng = np.random.default_rng(7)
    sets = [rng.integers(-50, 50, (n, 2)) for n in (1, 2, 3, 5, 9, 40)] + [rng.integers(-10 ** 6, 10 ** 6, (12, 2)), np.array([[0, 0], [5, 0], [9, 0]]),
                                                                          np.array([[0, 0], [6, 0], [6, 2], [2, 2], [2, 6], [0, 6]])]
    for pts in sets:
        p = np.ascontiguousarray(pts, np.int32)
        out = (C.c_float * 5)()
        assert _vp.lib().vp_min_area_rect_i32(p.ctypes.data, len(p), out) == 0
        assert np.array_equal(np.array(out[:], np.float32), R.min_area_rect(p)), pts.tolist()


def test_statement_perimeter_and_hull_agree_with_the_host_routines():
    from vision import _vp, cv2_facade
    rng = np.random.default_rng(11)
    for n in (1, 2, 3, 8, 70):
        p = np.ascontiguousarray(rng.integers(-300, 300, (n, 2)), np.int32)
        for closed in (True, False):
            assert R.perimeter(p, closed) == cv2_facade.arcLength(p, closed)
        out, k = np.empty_like(p), C.c_int(0)
        assert _vp.lib().vp_convex_hull_i32(p.ctypes.data, n, out.ctypes.data, C.byref(k)) == 0
        assert [tuple(v) for v in out[:k.value].tolist()] == R.hull(p)
