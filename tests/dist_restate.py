"""The statement of cv2.distanceTransform and cv2.minMaxLoc as this library defines them, twice and
independently in numpy: a brute-force minimum over all zero pixels, and a two-pass separable transform, both in integers.  Zero pixels
are the sources.  The integer maps are

  L2: D2 = min dx^2 + dy^2        L1: min |dx| + |dy|        C: min max(|dx|, |dy|)

with NONE (-1) everywhere when the image has no zero pixel, and the final values are np.sqrt(np.float32(D2)) (numpy's float32 root is
correctly rounded), np.float32 of the integers, np.minimum(d, 255).astype(np.uint8) - +inf / 255 for NONE."""
import numpy as np

L1, L2, C = 1, 2, 3
NONE = -1
METRICS = (L2, L1, C)


def _combine(metric, dy, dx):
    dy, dx = np.abs(dy), np.abs(dx)
    if metric == L2:
        return dy * dy + dx * dx
    if metric == L1:
        return dy + dx
    return np.maximum(dy, dx)


def brute(img, metric):
    """int64 (h, w): the minimum over all zero pixels, one zero pixel at a time in chunks"""
    img = np.asarray(img)
    h, w = img.shape
    zy, zx = np.nonzero(img == 0)
    if len(zy) == 0:
        return np.full((h, w), NONE, np.int64)
    yy, xx = np.indices((h, w), dtype=np.int64)
    best = np.full((h, w), np.iinfo(np.int64).max, np.int64)
    for i in range(0, len(zy), 256):
        dy = yy[None] - zy[i:i + 256, None, None]
        dx = xx[None] - zx[i:i + 256, None, None]
        best = np.minimum(best, _combine(metric, dy, dx).min(axis=0))
    return best


def separable(img, metric):
    """int64 (h, w): g(x, y) = horizontal distance to the nearest zero of row y by two running scans, then the minimum over rows"""
    img = np.asarray(img)
    h, w = img.shape
    big = 1 << 20                                       # "no zero in this row": above every distance, small enough to square
    g = np.full((h, w), big, np.int64)
    for y in range(h):
        d = big
        for x in range(w):
            d = 0 if img[y, x] == 0 else min(d + 1, big)
            g[y, x] = d
        d = big
        for x in range(w - 1, -1, -1):
            d = 0 if img[y, x] == 0 else min(d + 1, big)
            g[y, x] = min(g[y, x], d)
    if (g >= big).all():
        return np.full((h, w), NONE, np.int64)
    rows = np.arange(h, dtype=np.int64)
    out = np.empty((h, w), np.int64)
    for y in range(h):
        out[y] = _combine(metric, (rows - y)[:, None], g).min(axis=0)
    return out


def separable_fast(img, metric):
    """`separable` vectorised for the larger shapes of the GPU suite: the row scans by np.maximum.accumulate on zero positions, the
    column minimum by sweeping dy outwards over whole images"""
    img = np.asarray(img)
    h, w = img.shape
    big = 1 << 20
    xs = np.arange(w, dtype=np.int64)[None, :]
    zero = img == 0
    left = np.maximum.accumulate(np.where(zero, xs, -big), axis=1)
    right = np.minimum.accumulate(np.where(zero, xs, 2 * big)[:, ::-1], axis=1)[:, ::-1]
    g = np.minimum(np.minimum(xs - left, right - xs), big)
    if not zero.any():
        return np.full((h, w), NONE, np.int64)
    best = _combine(metric, 0, g)
    for dy in range(1, h):                              # rows dy above and below, until no pixel can still improve
        if (dy * dy if metric == L2 else dy) >= best.max():
            break
        cand = _combine(metric, dy, g)
        best[dy:] = np.minimum(best[dy:], cand[:-dy])
        best[:-dy] = np.minimum(best[:-dy], cand[dy:])
    return best


def reference(img, metric):
    """the integer map by whichever statement is quicker for the image (tests/test_dist_statement.py shows that they agree)"""
    return brute(img, metric) if 0 < np.count_nonzero(np.asarray(img) == 0) <= 64 else separable_fast(img, metric)


def finish(ints, metric, dtype=np.float32):
    """the integer map -> what distanceTransform returns"""
    none = ints == NONE
    if np.dtype(dtype) == np.uint8:
        assert metric == L1
        return np.where(none, 255, np.minimum(ints, 255)).astype(np.uint8)
    with np.errstate(invalid="ignore"):
        vals = np.sqrt(np.float32(np.where(none, 0, ints))) if metric == L2 else np.float32(ints)
    vals = np.asarray(vals, np.float32).copy()
    vals[none] = np.inf
    return vals


def distance_transform(img, metric, dtype=np.float32, how=reference):
    return finish(how(img, metric), metric, dtype)


def min_max_loc(a, mask=None):
    """(minVal, maxVal, (x, y), (x, y)): np.argmin / np.argmax on the raveled array over the pixels that take part - mask non-zero, not
    NaN - which return the first index among equals"""
    a = np.asarray(a)
    h, w = a.shape
    flat = a.ravel()
    part = np.ones(flat.shape, bool) if mask is None else (np.asarray(mask).ravel() != 0)
    if a.dtype.kind == "f":
        part &= ~np.isnan(flat)
    idx = np.nonzero(part)[0]
    if len(idx) == 0:
        return 0.0, 0.0, (-1, -1), (-1, -1)
    vals = flat[idx]
    lo, hi = int(idx[np.argmin(vals)]), int(idx[np.argmax(vals)])
    return float(flat[lo]), float(flat[hi]), (lo % w, lo // w), (hi % w, hi // w)


def largest_inscribed_circle(mask):
    _, radius, _, centre = min_max_loc(distance_transform(mask, L2))
    return centre, radius
