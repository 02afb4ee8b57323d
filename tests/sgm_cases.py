"""Seeded pairs and the one list of cases that the CPU statement test and the GPU test of semi-global matching both walk.  The pairs come
from the generators of tests/stereo_cases.py; the sizes that straddle a kernel's geometry come from vp_stereo_sgm_plan, not from
constants here.  Cases are small - at most 48 rows and num_disparities + 80 columns - except where a case says why it is not."""
import ctypes as C

import numpy as np

import sgm_restate as G
from stereo_cases import checker_columns, flat, shifted_pair, stripes, two_plane_pair

GEOMETRY = 15      # VP_SGM_GEOMETRY of include/vp.h


def lib_plan(w, h, n, block_size, m, paths=8):
    """vp_stereo_sgm_plan as a dict (host only: no device, no context)"""
    from vision import _vp
    rect, geom, ws = (C.c_int32 * 4)(), (C.c_int32 * GEOMETRY)(), C.c_size_t()
    _vp.check(_vp.lib().vp_stereo_sgm_plan(w, h, n, block_size, m, paths, rect, C.byref(ws), geom))
    g = list(geom)
    return dict(rect=tuple(rect), ws_bytes=ws.value,
                cost=dict(threads=g[0], strip_cols=g[1], grid=(g[2], g[3]), lds_bytes=g[4]),
                path=dict(threads=g[5], group=g[6], per_lane=g[7], lines_per_block=g[8], grid_h=g[9], grid_v=g[10], grid_d=g[11]),
                select=dict(threads=g[12], px_per_block=g[13], grid=g[14]))


def host_disparity(left, right, **params):
    """vp_stereo_sgm_host on packed arrays"""
    from vision import _vp
    p = G.resolve(params)
    h, w = left.shape
    out = np.empty((h, w), np.int16)
    _vp.check(_vp.lib().vp_stereo_sgm_host(left.ctypes.data, w, right.ctypes.data, w, w, h, *ordered(p), out.ctypes.data, 2 * w))
    return out


ORDER = ("num_disparities", "block_size", "min_disparity", "pre_filter_cap", "p1", "p2", "uniqueness_ratio", "disp12_max_diff", "paths")


def ordered(p):
    """the nine resolved parameters in the order of the C entries"""
    p = G.resolve(p)
    return tuple(p[k] for k in ORDER)


def size_for(cw, ch, n, block_size, m=0):
    """(h, w) of the smallest image whose candidate rectangle is cw x ch"""
    r = block_size // 2
    return ch + 2 * r, cw + 2 * r + max(m + n - 1, 0) + max(-m, 0)


def largest_p2(paths, cap, block_size):
    """the largest p2 the 16-bit bound admits"""
    return 65535 // paths - 2 * cap * block_size * block_size


def _case(cid, pair, oracle="statement", **params):
    return dict(id=cid, pair=pair, oracle=oracle, params={**G.DEFAULTS, **params})


def geometry_rects(plan, n):
    """candidate rectangles (cw, ch) that put the number of lines of a horizontal, a vertical and a diagonal direction, and the number of
    pixels, at a block boundary of the path and selection kernels, one below it and one above"""
    p = plan(200 + n, 40, n, 5, 0)
    out = []
    for v in {p["path"]["lines_per_block"] + k for k in (-1, 0, 1)}:
        if v >= 1:
            out += [(7, v), (v, 7), ((v + 1) // 2, v + 1 - (v + 1) // 2)]       # ch lines; cw lines; cw + ch - 1 lines
    for v in {p["select"]["px_per_block"] + k for k in (-1, 0, 1)}:
        out += [(v, 1), (1, v)]
    return sorted(set(out))


def cases(plan):
    """plan: lib_plan.  Each case: id, pair (a callable -> (left, right)), params (all nine, p1 / p2 possibly None), oracle."""
    out = []
    tiny = dict(num_disparities=16, block_size=5, uniqueness_ratio=0)
    # one candidate pixel; none; none; a single row; a single column; block_size 1 (r = 0)
    for name, (h, w), extra in (("one_pixel", (5, 20), {}), ("empty_w", (5, 19), {}), ("empty_h", (4, 40), {}), ("one_row", (5, 40), {}), ("one_column", (12, 20), {}),
                                ("block_1", (6, 30), dict(block_size=1, p1=2, p2=9))):
        out.append(_case(f"tiny_{name}", lambda h=h, w=w: shifted_pair(h, w, 1, 1), **{**tiny, **extra}))
    # fewer lanes than a wave, one wave, two and four disparities per lane - and the counts that leave lanes idle
    for n, all_paths in ((16, (4, 8)), (32, (4, 8)), (64, (4, 8)), (128, (4, 8)), (256, (4, 8)), (48, (8,)), (112, (8,)), (208, (8,))):
        for paths in all_paths:
            out.append(_case(f"nd_{n}_p{paths}", lambda n=n: shifted_pair(20, n + 60, n // 4 + 3, 5, noise=12), num_disparities=n, paths=paths))
    # diagonals that start on the top or bottom edge and on the side edges
    out.append(_case("tall", lambda: shifted_pair(48, 30, 4, 2, noise=12), num_disparities=16))
    out.append(_case("wide", lambda: shifted_pair(10, 90, 4, 2, noise=12), num_disparities=16))
    noisy = lambda: shifted_pair(36, 110, 10, 8, noise=40)
    for name, p1, p2 in (("zero", 0, 0), ("equal", 20, 20), ("p1_zero", 0, 50)):
        out.append(_case(f"penalty_{name}", noisy, num_disparities=32, p1=p1, p2=p2))
    for paths in (4, 8):        # costs saturate: S comes as near 65535 as the statement allows
        p2 = largest_p2(paths, 63, 5)
        out.append(_case(f"penalty_largest_p{paths}", lambda: (checker_columns(30, 80), checker_columns(30, 80, 2)), num_disparities=16, pre_filter_cap=63, p1=p2, p2=p2,
                         paths=paths, uniqueness_ratio=0))
    # |m| = 128 leaves no candidate column in an image narrower than 148: these two are 170 wide
    for m, w in ((-128, 170), (-3, 90), (4, 90), (128, 170)):
        out.append(_case(f"min_{m}", lambda m=m, w=w: shifted_pair(20, w, m + 7, 6, noise=12), num_disparities=16, min_disparity=m))
    for c in (1, 63):
        out.append(_case(f"cap_{c}", noisy, num_disparities=32, pre_filter_cap=c))
    out.append(_case("flat_ties", lambda: (flat(24, 70), flat(24, 70)), num_disparities=32, uniqueness_ratio=0))
    out.append(_case("flat_unique", lambda: (flat(24, 70), flat(24, 70)), num_disparities=32))
    out.append(_case("stripes_ties", lambda: (stripes(24, 100), stripes(24, 100)), num_disparities=32, uniqueness_ratio=0))
    for u in (0, 15, 100):
        out.append(_case(f"uniq_{u}", noisy, num_disparities=32, uniqueness_ratio=u, disp12_max_diff=-1))
    # the issue's pair for the left-right check; 160 columns
    for m in (0, 2):
        for diff in (-1, 0, 1, 255):
            out.append(_case(f"lr_m{m}_d{diff}", lambda: two_plane_pair(40, 160, 7), num_disparities=16, p1=8, p2=32, min_disparity=m, uniqueness_ratio=0,
                             disp12_max_diff=diff))
    strip = plan(200, 40, 16, 5, 0)["cost"]["strip_cols"]
    for cw in (strip - 1, strip, strip + 1, 2 * strip + 1):
        h, w = size_for(cw, 3, 16, 5)
        out.append(_case(f"strip_cw{cw}", lambda h=h, w=w: shifted_pair(h, w, 5, 2, noise=12), num_disparities=16))
    for n in (16, 32, 64):
        for cw, ch in geometry_rects(plan, n):
            h, w = size_for(cw, ch, n, 5)
            out.append(_case(f"geom_n{n}_{cw}x{ch}", lambda h=h, w=w, n=n: shifted_pair(h, w, n // 4, 3, noise=12), num_disparities=n))
    # the numpy statement is too slow for this size: its expectation is vp_stereo_sgm_host, which test_sgm_statement.py pins to the
    # statement on every small case
    out.append(_case("mid_640x360", lambda: shifted_pair(360, 640, 21, 9, noise=12), oracle="host"))
    return out


_expected = {}


def expected(case):
    """the expectation of a case, computed once per process and shared: treat it as read-only"""
    if case["id"] not in _expected:
        left, right = case["pair"]()
        out = host_disparity(left, right, **case["params"]) if case["oracle"] == "host" else G.disparity(left, right, **case["params"])
        out.setflags(write=False)
        _expected[case["id"]] = out
    return _expected[case["id"]]
