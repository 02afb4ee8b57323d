"""The statement of the contour-geometry pass in plain Python: what vp_contour_geometry_* and
vp_min_enclosing_circle_i32 are checked against.

  perimeter   float32 segment roots (numpy), added as Python integers of 2^-23 units
  hull        monotone chain on Python integers: strict vertices, from the smallest point, lower chain first
  rectangle   vision.cv2_facade._min_area_rect_loop, the statements vp_min_area_rect_i32 restates
  circle      brute force over all pairs and triples, every test in fractions.Fraction; centre and radius^2 are exact rationals,
              rounded to float32 at the very end (the root through exact integer square-root bracketing)
"""
import itertools
import math
from fractions import Fraction

import numpy as np

UNIT = 1 << 23


def perimeter_units(pts, closed=True):
    """the perimeter as an integer count of 2^-23: every float32 root of a lattice segment is such a count"""
    p = np.asarray(pts).reshape(-1, 2).astype(np.float32)
    if len(p) <= 1:
        return 0
    total = 0
    for i in range(0 if closed else 1, len(p)):
        d = p[i] - p[i - 1]
        root = np.sqrt(np.float32(d[0] * d[0] + d[1] * d[1]))
        units = Fraction(float(root)) * UNIT
        assert units.denominator == 1 and units < (1 << 40)
        total += int(units)
    return total


def perimeter(pts, closed=True):
    u = perimeter_units(pts, closed)
    assert u < (1 << 53)            # below that the sequential float64 sum is this number
    return u / UNIT


def hull(pts):
    """list of (x, y) integer tuples"""
    p = sorted(set((int(x), int(y)) for x, y in np.asarray(pts).reshape(-1, 2).tolist()))
    if len(p) <= 2:
        return p

    def cross(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    lower, upper = [], []
    for q in p:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], q) <= 0:
            lower.pop()
        lower.append(q)
    for q in reversed(p):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], q) <= 0:
            upper.pop()
        upper.append(q)
    return lower[:-1] + upper[:-1]


def hull_area2(h):
    return abs(sum(h[i][0] * h[(i + 1) % len(h)][1] - h[(i + 1) % len(h)][0] * h[i][1] for i in range(len(h))))


def min_area_rect(pts):
    """the five numbers (cx, cy, w, h, angle) as float32"""
    from vision import cv2_facade
    if len(np.asarray(pts).reshape(-1, 2)) == 0:
        return np.zeros(5, np.float32)
    (cx, cy), (w, h), ang = cv2_facade._min_area_rect_loop(np.asarray(pts).reshape(-1, 2))
    return np.array([cx, cy, w, h, ang], np.float32)


# ---- enclosing circle ---------------------------------------------------------------------------------------------------------

def support_circle(sup):
    """(cx, cy, r2) as Fractions of the circle 1..3 integer support points define: the point, the circle on the diameter, the
    circumcircle"""
    sup = [(int(x), int(y)) for x, y in sup]
    if len(sup) == 1:
        return Fraction(sup[0][0]), Fraction(sup[0][1]), Fraction(0)
    if len(sup) == 2:
        (ax, ay), (bx, by) = sup
        return Fraction(ax + bx, 2), Fraction(ay + by, 2), Fraction((ax - bx) ** 2 + (ay - by) ** 2, 4)
    (ax, ay), (bx, by), (cx, cy) = sup
    bx, by, cx, cy = bx - ax, by - ay, cx - ax, cy - ay
    d = 2 * (bx * cy - by * cx)
    assert d != 0
    ux = Fraction(cy * (bx * bx + by * by) - by * (cx * cx + cy * cy), d)
    uy = Fraction(bx * (cx * cx + cy * cy) - cx * (bx * bx + by * by), d)
    return ax + ux, ay + uy, ux * ux + uy * uy


def contains(circle, pts):
    cx, cy, r2 = circle
    return all((int(x) - cx) ** 2 + (int(y) - cy) ** 2 <= r2 for x, y in pts)


def min_enclosing_circle(pts):
    """(cx, cy, r2) as Fractions: the smallest circle over all single points, pairs and triples that contains every point"""
    p = sorted(set((int(x), int(y)) for x, y in np.asarray(pts).reshape(-1, 2).tolist()))
    if not p:
        return Fraction(0), Fraction(0), Fraction(0)
    if len(p) == 1:
        return support_circle(p)
    best = None
    for k in (2, 3):
        for sup in itertools.combinations(p, k):
            if k == 3 and (sup[1][0] - sup[0][0]) * (sup[2][1] - sup[0][1]) == (sup[1][1] - sup[0][1]) * (sup[2][0] - sup[0][0]):
                continue
            c = support_circle(sup)
            if (best is None or c[2] < best[2]) and contains(c, p):
                best = c
    return best


def round_f32(q):
    """the float32 nearest to the rational q (ties to even), as np.float32"""
    q = Fraction(q)
    if q == 0:
        return np.float32(0)
    s, a = (-1 if q < 0 else 1), abs(q)
    e = 0
    while a >= (1 << 24):
        a /= 2
        e += 1
    while a < (1 << 23):
        a *= 2
        e -= 1
    m = a.numerator // a.denominator
    rest = a - m
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and m % 2):
        m += 1
    return np.float32(s * math.ldexp(m, e))


def round_f32_sqrt(q):
    """the float32 nearest to sqrt(q) for a rational q >= 0: the 24-bit integer m with m <= sqrt(q) / 2^e < m + 1 by integer square
    root, then one exact comparison of q with the square of the midpoint"""
    q = Fraction(q)
    if q == 0:
        return np.float32(0)
    e = 0
    while q / Fraction(4) ** e >= (1 << 48):
        e += 1
    while q / Fraction(4) ** e < (1 << 46):
        e -= 1
    a = q / Fraction(4) ** e                                        # 2^46 <= a < 2^48: sqrt(a) in [2^23, 2^24)
    m = math.isqrt(a.numerator // a.denominator)
    while Fraction(m + 1) ** 2 <= a:
        m += 1
    mid = Fraction(2 * m + 1, 2) ** 2
    if a > mid or (a == mid and m % 2):
        m += 1
    return np.float32(math.ldexp(m, e))


def ulps(a, b):
    """distance of two float32 in units of the last place"""
    ia, ib = (int(np.array(v, np.float32).view(np.int32)) for v in (a, b))
    ia, ib = (v if v >= 0 else -(v & 0x7fffffff) for v in (ia, ib))
    return abs(ia - ib)


def circle_f32(circle):
    cx, cy, r2 = circle
    return round_f32(cx), round_f32(cy), round_f32_sqrt(r2)


def is_min_circle_of(sup, pts):
    """Whether the circle of the support points is the smallest enclosing circle of pts: it contains every point, and it is the
    smallest circle of its own support points (brute force over the at most three of them) - a smaller circle around all points
    would be a smaller one around those."""
    c = support_circle(sup)
    return contains(c, np.asarray(pts).reshape(-1, 2).tolist()) and min_enclosing_circle(sup)[2] == c[2]
