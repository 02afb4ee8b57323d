"""Inputs for the rectification and reprojection tests (tests/test_rectify_abi.py on the host statement, tests/test_gpu_rectify.py and
tests/test_gpu_reproject.py on the GPU): seeded images, fixed-form tables that reach every border rule, and the list of cases.  The
expected results come from tests/rectify_restate.py."""
import ctypes as C

import numpy as np

import rectify_restate as R
import remap_restate as RM

TABLES = ("outside", "edge_x", "edge_y", "identity", "lens")
Q_RIG = np.array([[1, 0, 0, -47.25], [0, 1, 0, -30.5], [0, 0, 0, 534.48], [0, 0, 1 / 0.12, 0]], np.float64)
Q_GENERAL = np.array([[1.01, 0.02, -0.3, -40.0], [-0.015, 0.99, 0.07, -28.0], [0.001, -0.002, 0.05, 500.0], [0.0003, 0.0002, 8.1, 0.37]], np.float64)
Q_ZERO_COLUMN = np.array([[1, 0, 0, -3.0], [0, 1, 0, -2.0], [0, 0, 0, 100.0], [1, 0, 0, -2.0]], np.float64)      # W = x - 2: column 2 is unknown


def plan(w=64, h=64, cn=3, ow=64, oh=64):
    """vp_rectify_pair_plan: tile columns, tile rows, pixels per lane, grid x, y, z"""
    from vision import _vp
    g = (C.c_int32 * 6)()
    _vp.check(_vp.lib().vp_rectify_pair_plan(w, h, cn, ow, oh, g))
    return dict(tile_w=g[0], tile_h=g[1], ppt=g[2], grid=(g[3], g[4], g[5]))


def image(h, w, cn, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w) if cn == 1 else (h, w, cn), dtype=np.uint8)


def table(kind, w, h, ow, oh, seed):
    """(xy int16 (oh, ow, 2), frac uint16 (oh, ow)) for a source of w x h pixels"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(ow), np.arange(oh))
    fr = (rng.integers(1, 32, (oh, ow)) * 32 + rng.integers(1, 32, (oh, ow))).astype(np.uint16)          # both fractions non-zero
    if kind == "outside":                        # every tap of every pixel lies outside: left of, right of, above or below the source
        pick = (x + y + seed) % 4                 # the nearest coordinates that leave no tap inside: -2 and w (h); the other one is free
        sx = np.where(pick == 0, -2, np.where(pick == 1, w, rng.integers(-3, w + 3, (oh, ow))))
        sy = np.where(pick == 2, -2, np.where(pick == 3, h, rng.integers(-3, h + 3, (oh, ow))))
    elif kind == "edge_x":                       # taps at column -1 (one inside neighbour: column 0) and w - 1 (one outside: column w)
        sx, sy = np.where((x + seed) % 2 == 0, -1, w - 1), (y + seed) % h
    elif kind == "edge_y":
        sx, sy = (x + seed) % w, np.where((y + x + seed) % 2 == 0, -1, h - 1)
    elif kind == "identity":
        sx, sy, fr = x + (seed % 2), y, np.zeros((oh, ow), np.uint16)                                     # the right table: one column over
    else:                                        # a 2 degree rotation about the centre with barrel distortion, as float maps -> convertMaps
        assert kind == "lens"
        a = np.deg2rad(2.0 if seed % 2 == 0 else -2.0)
        u, v = (x - (ow - 1) / 2) / max(ow, oh), (y - (oh - 1) / 2) / max(ow, oh)
        ur, vr = np.cos(a) * u - np.sin(a) * v, np.sin(a) * u + np.cos(a) * v
        k = 1 - 0.25 * (ur * ur + vr * vr)
        mx = (ur * k * max(w, h) * 1.1 + (w - 1) / 2 + 0.3 * (seed % 2)).astype(np.float32)
        my = (vr * k * max(w, h) * 1.1 + (h - 1) / 2).astype(np.float32)
        return RM.convert_maps_restate(mx, my)
    return np.ascontiguousarray(np.stack([sx, sy], axis=-1).astype(np.int16)), fr


def cases(tile_w, tile_h):
    out = []
    cns, keeps = (1, 3, 4), ("both", "left", "none")
    n = 0
    for ow in (tile_w - 1, tile_w, tile_w + 1):                                   # one row of tiles and one more, in each direction
        for oh in (tile_h - 1, tile_h, tile_h + 1):
            out.append(dict(w=61, h=37, cn=cns[n % 3], ow=ow, oh=oh, table="lens", keep=keeps[(n // 3) % 3]))
            n += 1
    for ow in (1, 3, 4, 5):                                                       # rows shorter than, equal to and just above a lane's group
        for oh in (1, 2):
            out.append(dict(w=5, h=3, cn=cns[n % 3], ow=ow, oh=oh, table=TABLES[n % 4], keep=keeps[n % 3]))
            n += 1
    for kind in TABLES:
        for cn in cns:
            out.append(dict(w=33, h=11, cn=cn, ow=40, oh=9, table=kind, keep="both"))
    for i, c in enumerate(out):
        c["seed"] = 100 + i
        c["id"] = f"{c['w']}x{c['h']}x{c['cn']}-to-{c['ow']}x{c['oh']}-{c['table']}-{c['keep']}"
    return out


def inputs(case):
    """(left, right, (xy, frac) left, (xy, frac) right): the two tables differ"""
    s = case["seed"]
    return (image(case["h"], case["w"], case["cn"], s), image(case["h"], case["w"], case["cn"], s + 1000),
            table(case["table"], case["w"], case["h"], case["ow"], case["oh"], 2 * s), table(case["table"], case["w"], case["h"], case["ow"], case["oh"], 2 * s + 1))


def expected(case):
    return R.rectify_pair(*inputs(case))


def reproject_cases():
    out = []
    rng = np.random.default_rng(7)
    special16 = np.array([-16, 0, 1, -1, 32767, -32768, 16, 800], np.int16)
    for w in (1, 3, 4, 5, 67):
        h = 3 if w < 67 else 45
        d16 = rng.integers(-64, 1024, (h, w)).astype(np.int16)
        d16.ravel()[:min(d16.size, special16.size)] = special16[:d16.size]
        f32 = (rng.random((h, w)) * 90 - 5).astype(np.float32)
        f32.ravel()[:min(f32.size, 5)] = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], np.float32)[:f32.size]
        for qname, q in (("rig", Q_RIG), ("general", Q_GENERAL), ("zero-column", Q_ZERO_COLUMN)):
            out.append(dict(id=f"i16-{w}x{h}-{qname}-invalid", disp=d16, Q=q, invalid=-16))
            out.append(dict(id=f"f32-{w}x{h}-{qname}", disp=f32, Q=q, invalid=None))
        out.append(dict(id=f"i16-{w}x{h}-rig-no-invalid", disp=d16, Q=Q_RIG, invalid=None))
    return out
