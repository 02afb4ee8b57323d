"""What a filled polygon is in this project, written down for the tests (no test in here).

The statement is vision/utils/draw.py: `draw_polylines(mat, pts, True, color, thickness < 0)` runs `_fill` - an even-odd scanline
whose crossings xa + (y - ya) * (xb - xa) / (yb - ya) are float64 - and then outlines the closed polygon with `_line` at thickness 1.
libvp (vp_fill_polys_u8 on the host, vp_fill_polys_dev in a kernel) computes the crossings as exact integers instead:

    key = (floor(crossing) + 32768) << 32  |  floor(2^32 * frac(crossing))

`spans_restate` is that arithmetic in Python integers.  Why it may replace the float64 one when every coordinate lies within
+-MAX_COORD = 32767: the denominators are at most 65534, so two different crossings differ by at least 1 / 65534^2 > 2^-32 - their keys
differ and order as they do - while the float64 value is off by at most a few ulp of 32768, below 2^-36: float64 orders different
crossings correctly, makes equal ones equal (or indistinguishable in what is painted), and cannot carry a non-integer over an integer,
so ceil and floor agree with the exact ones.  tests/test_fill_statement.py checks the claim against `_fill` itself.

`fill_poly_restate` is the statement of the cv2 stand-in's fillPoly: each polygon filled and outlined on its own, the image is the union
(cv2 itself runs one even-odd scanline over the edges of all polygons of a call: overlapping polygons differ, see cv2_facade.fillPoly).
"""
import numpy as np

from vision.utils import draw as D

MAX_COORD = 32767
MAX_CROSS = 256          # VP_FILL_MAX_CROSS: crossings per row the device kernel sorts


def cross_key(xa, ya, xb, yb, y):
    den, num = yb - ya, (y - ya) * (xb - xa)
    if den < 0:
        den, num = -den, -num
    fl, r = divmod(num, den)
    return ((xa + fl + 32768) << 32) | ((r << 32) // den)


def spans_restate(pts, h, w):
    """[(y, xa, xb)] in the order `_fill` paints them."""
    pts = [(int(x), int(y)) for x, y in np.asarray(pts).reshape(-1, 2)]
    n = len(pts)
    ys = [p[1] for p in pts]
    out = []
    for y in range(max(min(ys), 0), min(max(ys), h - 1) + 1):
        keys = []
        for i in range(n):
            (xa, ya), (xb, yb) = pts[i], pts[(i + 1) % n]
            if ya != yb and min(ya, yb) <= y < max(ya, yb):
                keys.append(cross_key(xa, ya, xb, yb, y))
        keys.sort()
        for a, b in zip(keys[0::2], keys[1::2]):
            xa = max((a >> 32) - 32768 + (1 if a & 0xFFFFFFFF else 0), 0)
            xb = min((b >> 32) - 32768, w - 1)
            if xa <= xb:
                out.append((y, xa, xb))
    return out


class SpanRecorder:
    """Stands in for the image `_fill` paints: keeps the spans instead of the pixels."""

    def __init__(self, h, w):
        self.shape = (h, w)
        self.spans = []

    def __setitem__(self, key, value):
        y, xs = key
        self.spans.append((int(y), int(xs.start), int(xs.stop) - 1))


def spans_of_fill(pts, h, w):
    rec = SpanRecorder(h, w)
    D._fill(rec, np.asarray(pts, np.int64).reshape(-1, 2), 1)
    return rec.spans


def statement(mat, polys, color):
    """The Python statement, polygon by polygon: `_fill`, then the closed outline at thickness 1 (what draw_polylines does when no
    native path takes the call)."""
    for p in polys:
        pts = np.asarray(p, np.int64).reshape(-1, 2)
        if len(pts) == 0:
            continue
        D._fill(mat, pts, color)
        if len(pts) == 1:
            D._line(mat, pts[0], pts[0], color, 1)
        for i in range(len(pts)):
            D._line(mat, pts[i], pts[(i + 1) % len(pts)], color, 1)


fill_poly_restate = statement


_coverage = {}


def coverage(name, h, w):
    """Boolean (h, w): the pixels the statement paints for CASES[name]; computed once per size and shared (read-only)."""
    k = (name, h, w)
    if k not in _coverage:
        m = np.zeros((h, w), np.uint8)
        statement(m, CASES[name], np.uint8(1))
        m = m.astype(bool)
        m.flags.writeable = False
        _coverage[k] = m
    return _coverage[k]


def expected(base, name, color):
    """`base` with CASES[name] painted in `color` by the statement."""
    out = base.copy()
    out[coverage(name, *base.shape[:2])] = color
    return out


def _star(cx, cy, r_out, r_in, tips):
    t = np.arange(2 * tips) * np.pi / tips
    r = np.where(np.arange(2 * tips) % 2 == 0, r_out, r_in)
    return np.stack([cx + r * np.sin(t), cy - r * np.cos(t)], 1).round().astype(np.int32)


def _comb(x0, step, teeth, y_top, y_bottom):
    """A zigzag of `teeth` downward teeth closed along the top: every row between the two levels is crossed 2 * teeth times."""
    xs = x0 + step * np.arange(2 * teeth + 1)
    ys = np.where(np.arange(2 * teeth + 1) % 2 == 0, y_top, y_bottom)
    return np.stack([xs, ys], 1).astype(np.int32)


# for images of 110 rows and 64 .. 200 columns
CASES = {
    "triangle": [np.array([[20, 10], [150, 40], [60, 100]], np.int32)],
    "star": [_star(100, 55, 50, 20, 5)],
    "bowtie": [np.array([[30, 20], [170, 90], [170, 20], [30, 90]], np.int32)],
    "vertex_on_scanline": [np.array([[10, 50], [40, 20], [70, 50], [100, 20], [130, 50], [70, 100]], np.int32)],      # local extrema and pass-through vertices
    "flat_top_bottom": [np.array([[30, 15], [120, 15], [140, 60], [100, 95], [50, 95], [20, 60]], np.int32)],
    "one_row": [np.array([[20, 33], [90, 33], [50, 33]], np.int32)],
    "one_point": [np.array([[77, 44]], np.int32)],
    "two_points": [np.array([[15, 12], [120, 75]], np.int32)],
    "integer_crossing": [np.array([[10, 10], [50, 50], [10, 90]], np.int32)],        # slope 1: every crossing is an integer, ceil == floor
    "half_crossing": [np.array([[10, 10], [31, 52], [11, 95], [5, 40]], np.int32)],
    "partly_left_top": [np.array([[-40, -30], [90, 20], [30, 80]], np.int32)],
    "partly_right_bottom": [np.array([[120, 60], [260, 90], [150, 160]], np.int32)],
    "outside_left": [np.array([[-90, 10], [-10, 20], [-50, 90]], np.int32)],
    "outside_right": [np.array([[210, 10], [290, 20], [250, 90]], np.int32)],
    "outside_above": [np.array([[10, -90], [100, -20], [50, -5]], np.int32)],
    "outside_below": [np.array([[10, 115], [100, 120], [50, 190]], np.int32)],
    "covers_everything": [np.array([[-50, -50], [400, -50], [400, 300], [-50, 300]], np.int32)],
    "comb": [_comb(-150, 2, 150, 10, 60)],                                          # 300 crossings on rows 10 .. 59: beyond MAX_CROSS
    # CHAIN_APPROX_SIMPLE contours of a blob with a hole, as cv2.findContours hands them out (the hole runs on the blob's pixels)
    "blob_with_hole": [np.array([[30, 20], [29, 21], [25, 21], [20, 26], [20, 70], [26, 76], [80, 76], [85, 71], [85, 30], [75, 20]], np.int32).reshape(-1, 1, 2),
                       np.array([[40, 40], [39, 41], [39, 55], [40, 56], [60, 56], [61, 55], [61, 41], [60, 40]], np.int32).reshape(-1, 1, 2)],
}
DEVICE_REFUSES = ("comb",)      # vp_fill_polys_dev: VP_ERR_CAPACITY, nothing painted
COLORS = {1: 180, 3: (7, 200, 255), 4: (1, 2, 3, 4)}
