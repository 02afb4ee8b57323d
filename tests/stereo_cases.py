"""Seeded image pairs for the stereo tests, and the one list of cases the CPU statement test and the GPU test both walk.  A pair obeys
the convention of tests/stereo_restate.py: the point of left (x, y) lies at right (x - D, y)."""
import numpy as np

import stereo_restate as R


def smooth_noise(h, w, seed=0):
    """uniform noise under a 3 x 3 mean: texture everywhere, neighbours correlated"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h + 2, w + 2)).astype(np.int32)
    s = sum(a[i:i + h, j:j + w] for i in range(3) for j in range(3))
    return (s // 9).astype(np.uint8)


def shifted_pair(h, w, d0, seed=0, noise=0):
    """(left, right) of one scene at disparity d0 everywhere (d0 may be negative); noise: the right image gets independent uniform noise
    of that amplitude on top, so that the best cost is not 0"""
    base = smooth_noise(h, w + abs(d0), seed)
    left, right = (base[:, :w], base[:, d0:d0 + w]) if d0 >= 0 else (base[:, -d0:-d0 + w], base[:, :w])
    if noise:
        extra = np.random.default_rng(seed + 1000).integers(-noise, noise + 1, (h, w))
        right = np.clip(right.astype(np.int32) + extra, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(left), np.ascontiguousarray(right)


def two_plane_pair(h, w, seed=0, near=11, far=5):
    """the left half of the right image sees the scene at disparity `far`, its right half at `near`"""
    left = smooth_noise(h, w + near, seed)
    right = np.empty((h, w), np.uint8)
    right[:, :w // 2] = left[:, far:far + w // 2]
    right[:, w // 2:] = left[:, near + w // 2:near + w]
    return np.ascontiguousarray(left[:, :w]), right


def flat(h, w, value=128):
    return np.full((h, w), value, np.uint8)


def stripes(h, w, period=8):
    """vertical stripes: every shift by a multiple of the period matches equally well"""
    row = np.where(np.arange(w) % period < period // 2, 255, 0).astype(np.uint8)
    return np.ascontiguousarray(np.broadcast_to(row, (h, w)))


def checker_columns(h, w, phase=0):
    """pairs of columns of 0 and of 255 in turn (the prefilter looks two columns apart): it saturates, at one end of its range or the
    other, in every interior pixel; phase 2 is the inverse image"""
    row = np.where(((np.arange(w) + phase) // 2) % 2 == 0, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.broadcast_to(row, (h, w)))


def _case(cid, pair, **params):
    return dict(id=cid, pair=pair, params={**R.DEFAULTS, **params})


def cases(plan):
    """plan(w, h, n, block_size, m) -> dict with strip_cols and band_rows (vp_stereo_bm_plan): the sizes that straddle the matcher's
    strip and band come from it, not from constants here.  Each case: id, pair (a callable -> (left, right)), params (all six)."""
    out = []
    small = dict(num_disparities=16, block_size=5)
    for h, w in ((5, 20), (5, 19), (4, 40), (7, 21)):                      # one candidate pixel; none; none; a 3 x 2 rectangle
        out.append(_case(f"tiny_{h}x{w}", lambda h=h, w=w: shifted_pair(h, w, 1, 1), **small, texture_threshold=0, uniqueness_ratio=0))
    for n, bs in ((16, 5), (256, 5)):                                      # both strip widths
        strip = plan(400, 40, n, bs, 0)["strip_cols"]
        for cw in (strip - 1, strip, strip + 1, 2 * strip):
            w = cw + 2 * (bs // 2) + n - 1
            out.append(_case(f"strip_n{n}_cw{cw}", lambda w=w, n=n: shifted_pair(7, w, n // 2, 2), num_disparities=n, block_size=bs))
    band = plan(60, 200, 16, 9, 0)["band_rows"]
    for h in (8, 9, 10, 8 + band, 9 + band):                               # no row, one, two (the first dropped row); one band, one above
        out.append(_case(f"rows_h{h}", lambda h=h: shifted_pair(h, 60, 6, 3), num_disparities=16, block_size=9))
    for bs in (5, 9, 15, 21):
        out.append(_case(f"block_{bs}", lambda: shifted_pair(48, 200, 9, 4), num_disparities=32, block_size=bs))
    for n in (16, 64, 128, 256):
        out.append(_case(f"nd_{n}", lambda n=n: shifted_pair(30, 330, n // 4 + 3, 5), num_disparities=n, block_size=9))
    for m in (-128, -3, 4, 128):
        out.append(_case(f"min_{m}", lambda m=m: shifted_pair(30, 330, m + 7, 6), num_disparities=16, block_size=7, min_disparity=m))
    for c in (1, 31, 63):                                                  # window sums of 441 * 2 c at every disparity that is a multiple of 4
        out.append(_case(f"cap_{c}", lambda: (checker_columns(30, 80), checker_columns(30, 80, 2)), num_disparities=16, block_size=21, pre_filter_cap=c,
                         uniqueness_ratio=0))
    out.append(_case("flat_t10", lambda: (flat(40, 120), flat(40, 120)), num_disparities=32, block_size=9))
    out.append(_case("flat_t0", lambda: (flat(40, 120), flat(40, 120)), num_disparities=32, block_size=9, texture_threshold=0))
    out.append(_case("stripes_u15", lambda: (stripes(40, 120), stripes(40, 120)), num_disparities=32, block_size=9))
    out.append(_case("stripes_ties", lambda: (stripes(40, 120), stripes(40, 120)), num_disparities=32, block_size=9, uniqueness_ratio=0))
    out.append(_case("two_planes", lambda: two_plane_pair(40, 160, 7), num_disparities=16, block_size=9))
    out.append(_case("uniq_0", lambda: shifted_pair(36, 150, 10, 8, noise=40), num_disparities=32, block_size=7, uniqueness_ratio=0))
    out.append(_case("uniq_100", lambda: shifted_pair(36, 150, 10, 8, noise=40), num_disparities=32, block_size=7, uniqueness_ratio=100))
    # every window clear of columns 0 and w - 1 has T = block_size^2 * cap exactly
    out.append(_case("texture_at", lambda: (checker_columns(24, 90), checker_columns(24, 90, 2)), num_disparities=16, block_size=7, uniqueness_ratio=0,
                     texture_threshold=49 * 31))
    out.append(_case("texture_above", lambda: (checker_columns(24, 90), checker_columns(24, 90, 2)), num_disparities=16, block_size=7, uniqueness_ratio=0,
                     texture_threshold=49 * 31 + 1))
    out.append(_case("hd720", lambda: shifted_pair(720, 1280, 21, 9)))
    return out


def lib_plan(w, h, n, block_size, m):
    """vp_stereo_bm_plan as a dict (host only: no device, no context)"""
    import ctypes as C
    from vision import _vp
    rect, geom, ws = (C.c_int32 * 4)(), (C.c_int32 * 5)(), C.c_size_t()
    _vp.check(_vp.lib().vp_stereo_bm_plan(w, h, n, block_size, m, rect, C.byref(ws), geom))
    return dict(rect=tuple(rect), ws_bytes=ws.value, strip_cols=geom[0], band_rows=geom[1], grid=(geom[2], geom[3]), lds_bytes=geom[4])


def host_disparity(left, right, **params):
    """vp_stereo_bm_host on packed arrays"""
    from vision import _vp
    p = {**R.DEFAULTS, **params}
    h, w = left.shape
    out = np.empty((h, w), np.int16)
    _vp.check(_vp.lib().vp_stereo_bm_host(left.ctypes.data, w, right.ctypes.data, w, w, h, p["num_disparities"], p["block_size"], p["min_disparity"],
                                          p["pre_filter_cap"], p["texture_threshold"], p["uniqueness_ratio"], out.ctypes.data, 2 * w))
    return out


_expected = {}


def expected(case):
    """the restatement's result of a case, computed once per process and shared: treat it as read-only"""
    if case["id"] not in _expected:
        left, right = case["pair"]()
        out = R.disparity(left, right, **case["params"])
        out.setflags(write=False)
        _expected[case["id"]] = out
    return _expected[case["id"]]
