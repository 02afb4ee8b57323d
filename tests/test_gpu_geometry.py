"""GPU suite for the contour-geometry pass (vp_contour_geometry_i32 / _dev / _batch_dev, vision.utils.feature.contour_geometry): every
row against the statement (tests/geometry_restate.py) and against the host routines it replaces - perimeter, hull vertices, hull area
and rectangle bit for bit, the circle within 1 float32 ulp of the correctly rounded circle of its support set (the margin is derived in
test_geometry_statement.py) and the support set exact: every point passes the statement's exact containment test and the support
circle is the smallest one of its own points.  Shapes are the smallest that reach every path: contours of 0, 1 and 2 points, a line,
a ring, speckle (hundreds of blocks), lane boundaries (63..257 points), the hull slot straddled by one, the batch entry with
max_contours straddled by one and a contour that overflows max_points."""
import ctypes as C

import numpy as np
import pytest

import geometry_restate as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from vision import _vp, cv2_facade
    from vision.utils import feature
    ctx = _vp.default_context()
    cap = C.c_int32(0)
    assert _vp.lib().vp_contour_geometry_plan(0, 0, 0, None, None, C.byref(cap)) == 0

    class Env:
        pass
    e = Env()
    e.vp, e.cv, e.feature, e.ctx, e.L, e.cap = _vp, cv2_facade, feature, ctx, _vp.lib(), cap.value
    return e


def _flat(contours):
    arrs = [np.asarray(c, np.int32).reshape(-1, 2) for c in contours]
    counts = np.array([len(a) for a in arrs], np.int32)
    flat = np.ascontiguousarray(np.concatenate(arrs) if arrs else np.zeros((0, 2)), np.int32).reshape(-1, 2)
    return flat, counts


def _raw_i32(e, contours, hulls=True):
    """rows of the ABI (support points included) and the hull block; the return code is checked"""
    flat, counts = _flat(contours)
    rows = np.zeros(len(counts), e.vp.CONTOUR_GEOM_DTYPE)
    hull = np.full_like(flat, -7)
    hc = np.full(len(counts), -1, np.int32)
    e.vp.check(e.L.vp_contour_geometry_i32(e.ctx.handle, flat.ctypes.data, counts.ctypes.data, len(counts), rows.ctypes.data,
                                           hull.ctypes.data if hulls else None, hc.ctypes.data), e.ctx.handle)
    assert np.array_equal(hc, rows["hull_count"])
    return rows, hull, flat, counts


class DevBuf:
    def __init__(self, e, a):
        self.e, self.p = e, C.c_void_p()
        e.vp.check(e.L.vp_dev_alloc(e.ctx.handle, max(a.nbytes, 8), C.byref(self.p)), e.ctx.handle)
        if a.nbytes:
            e.vp.check(e.L.vp_memcpy_h2d(e.ctx.handle, self.p, a.ctypes.data, a.nbytes), e.ctx.handle)

    def free(self):
        self.e.L.vp_dev_free(self.e.ctx.handle, self.p)


def _raw_dev(e, contours):
    flat, counts = _flat(contours)
    first = (np.cumsum(counts, dtype=np.int64) - counts).astype(np.int64)
    rows = np.zeros(len(counts), e.vp.CONTOUR_GEOM_DTYPE)
    bufs = [DevBuf(e, a) for a in (flat, first, counts)]
    try:
        e.vp.check(e.L.vp_contour_geometry_dev(e.ctx.handle, bufs[0].p, bufs[1].p, bufs[2].p, len(counts), rows.ctypes.data, None), e.ctx.handle)
    finally:
        for b in bufs:
            b.free()
    return rows


def _host_rect(e, p):
    out = (C.c_float * 5)()
    if len(p):
        assert e.L.vp_min_area_rect_i32(p.ctypes.data, len(p), out) == 0
    return np.array(out[:], np.float32)


def _host_hull(e, p):
    if len(p) == 0:
        return np.zeros((0, 2), np.int32)
    out, k = np.empty((max(len(p), 1), 2), np.int32), C.c_int(0)
    assert e.L.vp_convex_hull_i32(p.ctypes.data, len(p), out.ctypes.data, C.byref(k)) == 0
    return out[:k.value]


def _check_row(e, row, hull_block, pts, statement=True, want_status=0):
    """one row against the host routines (always) and the statement"""
    p = np.ascontiguousarray(pts, np.int32).reshape(-1, 2)
    assert row["status"] == want_status, (row["status"], len(p))
    assert row["perimeter"] == e.cv.arcLength(p, True) and row["perimeter_open"] == e.cv.arcLength(p, False)
    hh = _host_hull(e, p)
    assert row["hull_count"] == len(hh)
    if hull_block is not None:
        assert np.array_equal(hull_block[:len(hh)], hh)
    assert row["hull_area2"] == R.hull_area2([tuple(v) for v in hh.tolist()]) if len(hh) else row["hull_area2"] == 0
    assert row["rect"].tobytes() == _host_rect(e, p).tobytes(), (row["rect"], _host_rect(e, p), p.tolist()[:20])
    n = int(row["support_count"])
    sup = row["support"].reshape(3, 2)[:n].tolist()
    if len(p) == 0:
        assert n == 0 and not row["circle"].any()
        return
    assert 1 <= n <= 3 and all(tuple(s) in set(map(tuple, hh.tolist())) for s in sup)
    assert R.is_min_circle_of(sup, p.tolist()), (sup, p.tolist()[:20])
    want = R.circle_f32(R.support_circle(sup))
    assert all(R.ulps(g, w) <= 1 for g, w in zip(row["circle"], want)), (row["circle"], want)
    if statement:
        assert row["perimeter"] == R.perimeter(p, True) and row["perimeter_open"] == R.perimeter(p, False)
        assert [tuple(v) for v in hh.tolist()] == R.hull(p)
        assert row["rect"].tobytes() == R.min_area_rect(p).tobytes()
        if len(hh) <= 9:
            assert R.min_enclosing_circle(hh) == R.support_circle(sup)


def _check_all(e, contours, statement_every=1):
    rows, hull, flat, counts = _raw_i32(e, contours)
    o = 0
    for i, c in enumerate(counts.tolist()):
        _check_row(e, rows[i], hull[o:o + c], flat[o:o + c], statement=i % statement_every == 0)
        o += c
    # the Python table: the same numbers, the hull block as the ABI left it
    table, hb = e.feature.contour_geometry(contours, hulls=True)
    assert len(table) == len(rows)
    for name in ("perimeter", "perimeter_open", "hull_count", "rect", "circle", "status"):
        assert np.array_equal(table[name], rows[name]), name
    assert np.array_equal(table["hull_area"], rows["hull_area2"] * 0.5)
    o = 0
    for i, c in enumerate(counts.tolist()):
        assert np.array_equal(hb[o:o + rows["hull_count"][i]], hull[o:o + rows["hull_count"][i]])
        o += c
    return rows


def _mask(h, w):
    m = np.zeros((h, w), np.uint8)
    yy, xx = np.mgrid[:h, :w]
    m[(xx - w // 4) ** 2 + (yy - h // 3) ** 2 <= (min(h, w) // 5) ** 2] = 255               # a disc
    m[h // 2:h // 2 + 9, w // 2:w // 2 + 17] = 255                                             # a block ...
    m[h // 2 + 3:h // 2 + 6, w // 2 + 4:w // 2 + 12] = 0                                       # ... with a hole: a ring (RETR_LIST)
    m[2, 2] = 255                                                                               # one pixel
    m[2, 6:8] = 255                                                                             # two pixels
    m[h - 3, 5:w - 5] = 255                                                                     # a horizontal line: hull of 2 vertices
    m[h - 12:h - 6, w - 9:w - 2] = np.tri(6, 7, dtype=np.uint8) * 255                           # a triangle at the border
    return m


@pytest.mark.parametrize("h,w", [(48, 64), (131, 257)])
def test_small_masks(env, h, w):
    e = env
    cs = e.feature.find_contours(_mask(h, w), e.vp.RETR_LIST, e.vp.CHAIN_APPROX_SIMPLE)
    assert len(cs) >= 7
    rows = _check_all(e, cs)
    assert 1 in rows["hull_count"].tolist() and 2 in rows["hull_count"].tolist()
    line = rows[rows["hull_count"] == 2]
    assert (line["hull_area2"] == 0).all()
    cn = e.feature.find_contours(_mask(h, w), e.vp.RETR_LIST, e.vp.CHAIN_APPROX_NONE)     # every border pixel: more points per contour
    _check_all(e, cn)
    assert np.array_equal(e.feature.min_enclosing_rects(cs), rows["rect"]) and np.array_equal(e.feature.contour_perimeters(cs), rows["perimeter"])
    assert np.array_equal(e.feature.contour_perimeters(cs, closed=False), rows["perimeter_open"])


def test_speckle(env):
    e = env
    rng = np.random.default_rng(3)
    m = (rng.random((131, 257)) < 0.10).astype(np.uint8) * 255
    cs = e.feature.find_contours(m, e.vp.RETR_LIST, e.vp.CHAIN_APPROX_SIMPLE)
    assert len(cs) > 600
    _check_all(e, cs, statement_every=5)


def _rot(poly, deg, centre):
    a = np.deg2rad(deg)
    r = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    return np.rint((np.asarray(poly, np.float64) - centre) @ r.T + centre).astype(np.int32)


@pytest.mark.parametrize("deg", [0, 17, 45, 90, 133])
def test_drawn_shapes_at_rotations(env, deg):
    e = env
    from vision.utils import draw
    m = np.zeros((220, 220), np.uint8)
    c = np.array([110.0, 110.0])
    draw.draw_contours(m, [_rot([[60, 90], [160, 90], [160, 130], [60, 130]], deg, c).reshape(-1, 1, 2)], 255, -1)        # a rectangle
    cs = list(e.feature.find_contours(m, e.vp.RETR_EXTERNAL, e.vp.CHAIN_APPROX_SIMPLE))
    m[:] = 0
    draw.draw_circle(m, (110, 110), 40 + deg % 7, 255, -1)                                                                 # a disc
    cs += list(e.feature.find_contours(m, e.vp.RETR_EXTERNAL, e.vp.CHAIN_APPROX_SIMPLE))
    cs += list(e.feature.find_contours(m, e.vp.RETR_EXTERNAL, e.vp.CHAIN_APPROX_NONE))
    m[:] = 0
    ell = [[70, 70], [150, 70], [150, 100], [100, 100], [100, 150], [70, 150]]
    draw.draw_contours(m, [_rot(ell, deg, c).reshape(-1, 1, 2)], 255, -1)                                                  # an L
    cs += list(e.feature.find_contours(m, e.vp.RETR_EXTERNAL, e.vp.CHAIN_APPROX_SIMPLE))
    assert len(cs) == 4 and min(len(x) for x in cs) >= 4
    _check_all(e, cs)


def test_first_edge_wins_a_tie(env):
    """an L whose smallest rectangle is reached by several hull edges (every axis-parallel one, area 36): the first in hull order
    decides width, height and angle - the quarter turns start the hull at different corners"""
    e = env
    ell = np.array([[0, 0], [6, 0], [6, 2], [2, 2], [2, 6], [0, 6]], np.int32)
    turns = [ell, ell[:, ::-1] * [-1, 1], -ell, ell[:, ::-1] * [1, -1], ell + [100, -50]]
    rows = _check_all(e, [t.reshape(-1, 1, 2) for t in turns])
    for row in rows:
        assert row["hull_count"] == 5 and float(row["rect"][2]) * float(row["rect"][3]) == 36.0


def _convex_polygon(n):
    """a convex lattice polygon of exactly n vertices, every point a strict hull vertex: the n shortest primitive vectors (with their
    negatives), sorted by angle, added up"""
    from math import atan2, gcd
    vs = sorted(((x, y) for x in range(-40, 41) for y in range(-40, 41) if gcd(abs(x), abs(y)) == 1), key=lambda v: (v[0] ** 2 + v[1] ** 2, v))
    half = [v for v in vs if v[1] > 0 or (v[1] == 0 and v[0] > 0)]
    use = half[:(n + 1) // 2]
    use = use + [(-x, -y) for x, y in use]
    if n % 2:                                     # an odd count: two neighbours of the sorted fan are replaced by their sum
        use.sort(key=lambda v: atan2(v[1], v[0]))
        a, b = use[0], use[1]
        use = [(a[0] + b[0], a[1] + b[1])] + use[2:]
    use.sort(key=lambda v: atan2(v[1], v[0]))
    pts = np.cumsum(np.array(use, np.int64), axis=0)
    pts -= (pts.max(0) + pts.min(0)) // 2
    assert len(pts) == n and np.abs(pts).max() < 32768 and len(R.hull(pts)) == n
    return pts.astype(np.int32)


def test_hull_slot_straddled_by_one(env):
    e = env
    cap = e.cap
    rng = np.random.default_rng(5)
    polys = {n: _convex_polygon(n) for n in (cap - 1, cap, cap + 1)}
    rows, hull, flat, counts = _raw_i32(e, [polys[cap - 1], polys[cap], polys[cap + 1]])
    assert rows["status"].tolist() == [0, 0, e.vp.GEOM_HULL_CAP], "the overflow is reported, never silent"
    assert rows["hull_count"].tolist() == [cap - 1, cap, cap + 1]
    o = 0
    for i, n in enumerate((cap - 1, cap, cap + 1)):
        _check_row(e, rows[i], hull[o:o + n], polys[n], statement=(i == 0), want_status=rows["status"][i])
        o += n
    # the device forms leave such a row for the caller, with its perimeter
    dev = _raw_dev(e, [polys[cap], polys[cap + 1]])
    assert dev["status"].tolist() == [0, e.vp.GEOM_HULL_CAP] and dev[1]["hull_count"] == 0 and not dev[1]["rect"].any()
    assert dev[0].tobytes() == rows[1].tobytes() and dev[1]["perimeter"] == rows[2]["perimeter"]
    # the Python table comes back complete and equal, whatever the order of the points and with every point twice
    table, hb = e.feature.contour_geometry([polys[cap + 1].reshape(-1, 1, 2)], hulls=True)
    assert table["hull_count"][0] == cap + 1 and np.array_equal(table["rect"][0], rows[2]["rect"]) and np.array_equal(table["circle"][0], rows[2]["circle"])
    base = polys[cap - 1]
    shuffled = base[rng.permutation(len(base))]
    doubled = np.repeat(base, 2, axis=0)
    r2, h2, _, c2 = _raw_i32(e, [shuffled, doubled, np.concatenate([shuffled[:40], doubled])])
    want = _host_hull(e, base)
    o = 0
    for i, c in enumerate(c2.tolist()):
        assert r2["hull_count"][i] == cap - 1 and np.array_equal(h2[o:o + cap - 1], want), i
        for name in ("hull_area2", "rect", "circle"):
            assert np.array_equal(r2[name][i], rows[name][0]), (i, name)
        o += c
    assert r2["status"].tolist() == [0, e.vp.GEOM_HULL_CAP, e.vp.GEOM_HULL_CAP]     # twice the candidates pass the slot: finished by the host routines


def test_lane_and_block_boundaries(env):
    e = env
    rng = np.random.default_rng(9)
    sizes = [63, 64, 65, 255, 256, 257]
    cs = [rng.integers(-90, 90, (n, 2)).astype(np.int32) for n in sizes]
    cs += [np.stack([np.arange(n), (np.arange(n) * 7) % 5], 1).astype(np.int32) for n in (64, 65)]     # few interior points: nearly all survive the octagon
    _check_all(e, cs)
    for k in (1, 4, 5):
        _check_all(e, [rng.integers(0, 30, (5 + i, 2)).astype(np.int32) for i in range(k)])
    rows, hull, flat, counts = _raw_i32(e, [])
    assert len(rows) == 0
    table = e.feature.contour_geometry([])
    assert table.shape == (0,) and table.dtype == e.feature.GEOMETRY_DTYPE
    # an empty contour among others: zeros, status ok
    rows = _check_all(e, [np.zeros((0, 2), np.int32), np.array([[3, 4]], np.int32), np.zeros((0, 2), np.int32), np.array([[1, 1], [5, 4]], np.int32)])
    assert rows["hull_count"].tolist() == [0, 1, 0, 2] and rows[0].tobytes() == bytes(80)


def test_long_segments_reach_the_perimeter_bound(env):
    """12000 segments across the whole coordinate range: the total passes 2^53 units, the row says so and carries the sequential sum"""
    e = env
    n = 12000
    z = np.empty((n, 2), np.int32)
    z[0::2] = [-32768, -32768]
    z[1::2] = [32767, 32767]
    z[:, 0] += (np.arange(n) % 3).astype(np.int32) * np.where(np.arange(n) % 2 == 0, 1, -1)
    rows, hull, flat, counts = _raw_i32(e, [z, z[:4000]])
    assert R.perimeter_units(z[:200]) * (n // 200) > (1 << 53) * 0.99
    # (every point is a hull candidate here, so the hull slot overflows as well: both bits are reported)
    assert (rows["status"] & e.vp.GEOM_PERIMETER).tolist() == [e.vp.GEOM_PERIMETER, 0]
    assert rows[0]["perimeter"] == e.cv.arcLength(z, True) and rows[0]["perimeter_open"] == e.cv.arcLength(z, False)
    assert rows[1]["perimeter"] == e.cv.arcLength(z[:4000], True) == R.perimeter(z[:4000], True)
    assert rows[0]["rect"].tobytes() == _host_rect(e, z).tobytes() and rows[0]["hull_count"] == len(_host_hull(e, z))
    dev = _raw_dev(e, [z])
    assert dev["status"][0] & e.vp.GEOM_PERIMETER and dev["perimeter"][0] == 0 and dev["perimeter_open"][0] == 0


def test_device_form_flags_a_coordinate_outside_the_bound(env):
    e = env
    rows = _raw_dev(e, [np.array([[0, 0], [5, 5], [40000, 2]], np.int32), np.array([[0, 0], [5, 5], [4, 2]], np.int32)])
    assert rows["status"].tolist() == [e.vp.GEOM_COORD, 0] and rows[0]["perimeter"] == 0 and rows[0]["hull_count"] == 0
    # the Python layer takes such a list through the host routines
    table = e.feature.contour_geometry([np.array([[0, 0], [5, 5], [40000, 2]], np.int32)])
    assert table["perimeter"][0] == e.cv.arcLength(np.array([[0, 0], [5, 5], [40000, 2]], np.int32), True) and table["hull_count"][0] == 3


def test_batch_entry_on_a_chain_runner(env):
    e = env
    from vision.utils.chain import ChainRunner
    h, w, mc, mp = 48, 64, 3, 40
    frames = np.zeros((3, h, w, 3), np.uint8)

    def blob(f, y, x, hh, ww):
        frames[f, y:y + hh, x:x + ww] = 255
    blob(0, 4, 4, 5, 7); blob(0, 20, 30, 3, 3)                                              # max_contours - 1
    blob(1, 4, 4, 2, 2); blob(1, 10, 40, 1, 1); blob(1, 30, 10, 4, 9)                       # max_contours
    blob(2, 2, 2, 3, 3); blob(2, 8, 8, 17, 20); blob(2, 30, 40, 2, 5); blob(2, 40, 5, 3, 3)  # max_contours + 1; the second one has 70 border pixels
    runner = ChainRunner(3, h, w, e.vp.BGR2GRAY, (128, 0, 0), (255, 255, 255), morph=(), ccl=0, want=("threshed",),
                         contours=dict(source="threshed", mode=e.vp.RETR_EXTERNAL, method=e.vp.CHAIN_APPROX_NONE, max_contours=mc, max_points=mp))
    runner.input[:] = frames
    runner.run()
    arrs = {k: np.array(v) for k, v in runner.carrs.items()}
    assert arrs["info"][:, 0].tolist() == [2, 3, 4]
    # nothing is read beyond info: rows of counts / offsets that hold no contour are made unusable
    for f in range(3):
        k = min(int(arrs["info"][f, 0]), mc)
        arrs["counts"][f, k:] = 1 << 30
        arrs["offsets"][f, k:] = -5
    table = e.feature.contour_geometry(arrs)
    assert table.shape == (3, mc)
    traced = 0
    for f in range(3):
        k = min(int(arrs["info"][f, 0]), mc)
        for r in range(mc):
            cnt, off = int(arrs["counts"][f, r]), int(arrs["offsets"][f, r])
            if r >= k or cnt <= 0 or off + cnt > mp:
                assert table["status"][f, r] == e.vp.GEOM_SKIPPED and table[f, r]["perimeter"] == 0 and not table[f, r]["rect"].any(), (f, r)
                continue
            traced += 1
            pts = arrs["points"][f, off:off + cnt]
            one = e.feature.contour_geometry([pts.reshape(-1, 1, 2)])[0]
            assert table[f, r].tobytes() == one.tobytes(), (f, r)
    assert traced >= 6 and (table["status"][2] == e.vp.GEOM_SKIPPED).sum() >= 1, "frame 2 holds the contour that overflowed max_points"


def test_three_forms_agree_byte_for_byte(env):
    e = env
    rng = np.random.default_rng(21)
    mc, mp, n = 5, 96, 2
    info = np.zeros((n, 2), np.int32)
    counts = np.zeros((n, mc), np.int32)
    offsets = np.zeros((n, mc), np.int32)
    points = np.zeros((n, mp, 2), np.int32)
    cs = []
    for f, sizes in enumerate([(1, 2, 30, 9), (17, 3, 64)]):
        o = 0
        for r, s in enumerate(sizes):
            p = rng.integers(-500, 500, (s, 2)).astype(np.int32)
            points[f, o:o + s], counts[f, r], offsets[f, r] = p, s, o
            cs.append(p)
            o += s
        info[f] = (len(sizes), o)
    a, _, _, _ = _raw_i32(e, cs, hulls=False)
    b = _raw_dev(e, cs)
    assert a.tobytes() == b.tobytes()
    cd = e.vp.make_contour_desc(max_contours=mc, max_points=mp)
    cb = e.vp.ContourBuffers()
    bufs = {k: DevBuf(e, v) for k, v in (("info", info), ("counts", counts), ("offsets", offsets), ("points", points))}
    rows = np.zeros((n, mc), e.vp.CONTOUR_GEOM_DTYPE)
    try:
        for k, v in bufs.items():
            setattr(cb, k, v.p.value)
        e.vp.check(e.L.vp_contour_geometry_batch_dev(e.ctx.handle, C.byref(cd), C.byref(cb), n, rows.ctypes.data), e.ctx.handle)
    finally:
        for v in bufs.values():
            v.free()
    got = np.concatenate([rows[0, :4], rows[1, :3]])
    assert got.tobytes() == a.tobytes()
    assert (rows[0, 4:]["status"] == e.vp.GEOM_SKIPPED).all() and (rows[1, 3:]["status"] == e.vp.GEOM_SKIPPED).all()
