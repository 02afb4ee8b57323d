"""The statement of semi-global stereo matching, in numpy: what vp_stereo_sgm_* must equal byte for byte.  It
follows Hirschmueller's semi-global matching and the shape of cv2.StereoSGBM; where the text below fixes a rule, the rule is the contract:
it does not claim OpenCV's bits.  Prefilter, cost, candidate rectangle and invalid value are those of tests/stereo_restate.py.

  cost        C(x, y, d), d in [0, n), D = m + d: stereo_restate.cost_volume over its candidate rectangle (valid_rect at this block_size),
              cw x ch; everything outside is INV = (m - 1) * 16; there is no texture test
  paths       directions of travel (dy, dx): (0, 1), (0, -1), (1, 0), (-1, 0); paths = 8 adds (1, 1), (1, -1), (-1, 1), (-1, -1).
              For p whose predecessor q = p - (dy, dx) lies outside the rectangle L(p, d) = C(p, d); else, with M = min over k of L(q, k),
              L(p, d) = C(p, d) + min(L(q, d), L(q, d-1) + p1, L(q, d+1) + p1, M + p2) - M; a term whose d -+ 1 leaves [0, n) is absent
  sum         S = the sum of L over the paths, exact integers; paths * (2 c block_size^2 + p2) <= 65535 keeps it in 16 bits
  best        d* minimises S, ties to the larger d
  uniqueness  (ratio > 0 only) t = S* + S* ratio // 100; any d with |d - d*| > 1 and S(d) <= t gives INV
  left-right  (disp12_max_diff >= 0 only) xr = x - (m + d*); the right view's answer there is the d in [0, n) that minimises
              S(xr + m + d, y, d) over the d whose column xr + m + d is a candidate column, ties to the larger d (d* is always among
              them); |d_right - d*| > disp12_max_diff gives INV.  The integer d*, not the subpixel value.
  subpixel    the parabola rule of stereo_restate.py on S, pm and pp mirrored at the ends of the range; int16 (D* 256 + off + 15) >> 4
"""
import numpy as np

from stereo_restate import cost_volume, invalid_disparity, prefilter, valid_rect  # noqa: F401  (prefilter, valid_rect: the statement's parts, for its readers)

DIRECTIONS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1))
DEFAULTS = dict(num_disparities=64, block_size=5, min_disparity=0, pre_filter_cap=31, p1=None, p2=None, uniqueness_ratio=10, disp12_max_diff=1, paths=8)
BIG = 1 << 40


def resolve(params):
    """all nine parameters as integers: p1=None is 8 block_size^2, p2=None is 32 block_size^2"""
    p = {**DEFAULTS, **params}
    bs = p["block_size"]
    p["p1"] = 8 * bs * bs if p["p1"] is None else p["p1"]
    p["p2"] = 32 * bs * bs if p["p2"] is None else p["p2"]
    return p


def admitted(p):
    n, bs, m, c = p["num_disparities"], p["block_size"], p["min_disparity"], p["pre_filter_cap"]
    return (16 <= n <= 256 and n % 16 == 0 and bs % 2 == 1 and 1 <= bs <= 9 and -128 <= m <= 128 and 1 <= c <= 63 and 0 <= p["p1"] <= p["p2"]
            and 0 <= p["uniqueness_ratio"] <= 100 and -1 <= p["disp12_max_diff"] <= 255 and p["paths"] in (4, 8)
            and p["paths"] * (2 * c * bs * bs + p["p2"]) <= 65535)


def _step(Cp, Lq, p1, p2):
    """L of a line of pixels from their predecessors' L: Cp, Lq of shape (k, n)"""
    M = Lq.min(axis=1, keepdims=True)
    down = np.full_like(Lq, BIG)
    up = np.full_like(Lq, BIG)
    down[:, 1:] = Lq[:, :-1] + p1
    up[:, :-1] = Lq[:, 1:] + p1
    return Cp + np.minimum(np.minimum(Lq, M + p2), np.minimum(down, up)) - M


def path_costs(C, dy, dx, p1, p2):
    """L of one direction over the whole rectangle; C of shape (ch, cw, n), int64"""
    ch, cw, n = C.shape
    L = np.empty_like(C)
    if dy == 0:                                                    # a whole column per step
        xs = range(cw) if dx > 0 else range(cw - 1, -1, -1)
        for i, x in enumerate(xs):
            L[:, x] = C[:, x] if i == 0 else _step(C[:, x], L[:, x - dx], p1, p2)
        return L
    ys = range(ch) if dy > 0 else range(ch - 1, -1, -1)
    for i, y in enumerate(ys):                                     # a whole row per step
        L[y] = C[y]
        if i == 0:
            continue
        q = L[y - dy]
        if dx == 0:
            L[y] = _step(C[y], q, p1, p2)
        elif dx > 0:                                               # column 0 has no predecessor
            L[y, 1:] = _step(C[y, 1:], q[:-1], p1, p2)
        else:                                                      # nor has column cw - 1
            L[y, :-1] = _step(C[y, :-1], q[1:], p1, p2)
    return L


def summed_costs(left, right, **params):
    """(S of shape (ch, cw, n) as int64, rect) over the candidate rectangle; None when it is empty"""
    p = resolve(params)
    assert admitted(p), p
    cv = cost_volume(left, right, p["num_disparities"], p["block_size"], p["min_disparity"], p["pre_filter_cap"])
    if cv is None:
        return None
    C = np.ascontiguousarray(cv[0].transpose(1, 2, 0)).astype(np.int64)
    S = np.zeros_like(C)
    for dy, dx in DIRECTIONS[:p["paths"]]:
        S += path_costs(C, dy, dx, p["p1"], p["p2"])
    return S, cv[2]


def _last_argmin(a):
    """along the last axis, ties to the larger index"""
    return a.shape[-1] - 1 - np.argmin(a[..., ::-1], axis=-1)


def disparity(left, right, **params):
    left, right = np.asarray(left), np.asarray(right)
    assert left.dtype == np.uint8 and right.dtype == np.uint8 and left.ndim == 2 and left.shape == right.shape
    p = resolve(params)
    n, m = p["num_disparities"], p["min_disparity"]
    h, w = left.shape
    out = np.full((h, w), invalid_disparity(m), np.int16)
    sc = summed_costs(left, right, **p)
    if sc is None:
        return out
    S, (x0, y0, cw, ch) = sc
    assert S.max() <= 65535
    ds = _last_argmin(S)
    take = lambda d: np.take_along_axis(S, d[..., None], axis=-1)[..., 0]
    smin = take(ds)
    keep = np.ones((ch, cw), bool)
    if p["uniqueness_ratio"] > 0:
        limit = smin + smin * p["uniqueness_ratio"] // 100
        far = np.abs(np.arange(n)[None, None, :] - ds[..., None]) > 1
        keep &= ~np.any(far & (S <= limit[..., None]), axis=-1)
    if p["disp12_max_diff"] >= 0:
        # the right view at candidate column u (of the right image, u = xc - d for the left candidate xc = u + d) answers with the d that
        # minimises S(u + d, y, d); the left pixel x looks at u = x - d*
        xs = np.arange(cw)[None, :, None] - ds[..., None] + np.arange(n)[None, None, :]            # candidate column of each d's entry
        inside = (xs >= 0) & (xs < cw)
        along = np.where(inside, S[np.arange(ch)[:, None, None], np.clip(xs, 0, cw - 1), np.arange(n)[None, None, :]], BIG)
        keep &= np.abs(_last_argmin(along) - ds) <= p["disp12_max_diff"]
    pm = take(np.where(ds > 0, ds - 1, ds + 1))
    pp = take(np.where(ds < n - 1, ds + 1, ds - 1))
    num = (pm - pp) * 256
    den = pm + pp - 2 * smin + np.abs(pm - pp)
    off = np.where(den == 0, 0, np.sign(num) * (np.abs(num) // np.maximum(den, 1)))                # C's division: towards zero
    val = ((m + ds) * 256 + off + 15) >> 4
    out[y0:y0 + ch, x0:x0 + cw] = np.where(keep, val, invalid_disparity(m)).astype(np.int16)
    return out
