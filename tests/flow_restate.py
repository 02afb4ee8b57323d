"""The statement of cv2.calcOpticalFlowPyrLK as this library defines it, in numpy: the oracle of
tests/test_gpu_flow.py.  The product never imports this file.  The GPU must equal it bit for bit in nextPts, status and err.

OpenCV keeps the window of the first image and its Scharr derivatives as int16, takes fixed-point bilinear samples (W_BITS = 14) and
accumulates sums of integer products in float32 SIMD order.  Here those sums are exact integers; what follows them is OpenCV's
sequence of steps, in double in the one order written below, rounded to float32 where OpenCV holds a float.

  pyramid   level 0 is the image, level l + 1 = pyrDown(level l, BORDER_REFLECT_101) (box_pyr_restate.pyr_down_restate).  Level l
            exists while its width is above the window's and its height above the window's; the effective maxLevel is the last
            existing level at or below the requested one; level 0 must exist.
  values    outside a level an image value is BORDER_REFLECT_101; the derivative pair is calcSharrDeriv's ([3 10 3] across [-1 0 1],
            unscaled, reflect-101 at the level's edge) inside the level and 0 outside it.
  float32   the points, prevPt = pts * (float)(1 / 2^level), halfWin = (win - 1) * 0.5f, every nextPt, a, b, the three products
            under cvRound, delta (rounded once from double), nextPt += delta, delta + prevDelta, delta * 0.5f, minEig and err.
  double    A = S * 2^-20 and b = B * 2^-20 (exact), D = A11 * A22 - A12 * A12,
            minEig = ((A22 + A11) - sqrt((A11 - A22) * (A11 - A22) + 4 * (A12 * A12))) / (2 * ww * wh) -> float32,
            lost when (double)minEig < minEigThreshold or D < FLT_EPSILON,
            delta = (((A12 * b2) - (A22 * b1)) / D, ((A12 * b1) - (A11 * b2)) / D) -> float32,
            stop when (double)dx * dx + (double)dy * dy <= eps * eps, or when j > 0 and both |delta + prevDelta| (a float32 sum) < 0.01,
            err = (float)((double)sum|diff| / (double)(32 * ww * wh)).
  deviations  err is 0 whenever status is 0 and the minimum-eigenvalue flag is off; a point (or, with OPTFLOW_USE_INITIAL_FLOW, a guess)
            with a coordinate that is not finite or beyond +-2^24 gets status 0, err 0 and the position it would have started from
            echoed.  Every range test is made on the floored float before any conversion to an integer."""
import numpy as np

from box_pyr_restate import pyr_down_restate

OPTFLOW_USE_INITIAL_FLOW = 4
OPTFLOW_LK_GET_MIN_EIGENVALS = 8
W_BITS = 14
FLT_EPSILON = 1.1920928955078125e-07
COORD_LIMIT = 16777216.0
f32 = np.float32


def texture(h, w, seed=1, shift=(0.0, 0.0), waves=24, top=0.35):
    """A band-limited random texture, uint8 (h, w): a sum of `waves` cosines of spatial frequencies below `top` radians per pixel,
    evaluated at (x - shift[0], y - shift[1]) - so a shifted copy is the same function sampled elsewhere, not an interpolation."""
    r = np.random.default_rng(seed)
    fx, fy = r.uniform(-top, top, waves), r.uniform(-top, top, waves)
    ph, am = r.uniform(0, 2 * np.pi, waves), r.uniform(0.5, 1.0, waves)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = x - shift[0], y - shift[1]
    v = sum(a * np.cos(u * x + q * y + p) for a, u, q, p in zip(am, fx, fy, ph))
    # the scale comes from the amplitudes, not from the samples: the shifted copy is quantised alike
    return np.rint(np.clip(v / am.sum() * 1.5 + 0.5, 0, 1) * 255).astype(np.uint8)


def level_count(w, h, ww, wh, max_level):
    """existing levels among 0 .. max_level (0: level 0 itself is not larger than the window)"""
    n = 0
    while n <= max_level and n < 16 and w > ww and h > wh:
        n, w, h = n + 1, (w + 1) // 2, (h + 1) // 2
    return n


def build_levels(img, ww, wh, max_level):
    img = np.ascontiguousarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    n = level_count(img.shape[1], img.shape[0], ww, wh, max_level)
    if n == 0:
        raise ValueError("the image must be larger than the window")
    out = [img]
    while len(out) < n:
        out.append(pyr_down_restate(out[-1]))
    return out


def scharr_deriv(img):
    """(Ix, Iy) int64 of calcSharrDeriv: smoothing [3 10 3] across the difference [-1 0 1], reflect-101 at the edge"""
    p = np.pad(img.astype(np.int64), 1, mode="reflect")
    t0 = 3 * (p[:-2] + p[2:]) + 10 * p[1:-1]
    t1 = p[2:] - p[:-2]
    return t0[:, 2:] - t0[:, :-2], 3 * (t1[:, 2:] + t1[:, :-2]) + 10 * t1[:, 1:-1]


def descale(x, n):
    return (x + (1 << (n - 1))) >> n


def weights(a, b):
    """the four fixed-point bilinear weights of the float32 fractions a (x) and b (y); cvRound rounds half to even"""
    one, s = f32(1), f32(1 << W_BITS)
    iw00 = int(np.rint((one - a) * (one - b) * s))
    iw01 = int(np.rint(a * (one - b) * s))
    iw10 = int(np.rint((one - a) * b * s))
    return iw00, iw01, iw10, (1 << W_BITS) - iw00 - iw01 - iw10


class _Level:
    """one level of both pyramids, padded by the window so that a window the range test admits is a plain slice"""

    def __init__(self, prev, nxt, ww, wh):
        self.rows, self.cols = prev.shape
        pad = ((wh, wh), (ww, ww))         # the range test admits -win .. side - 1, and a window reaches win pixels further
        self.I = np.pad(prev.astype(np.int64), pad, mode="reflect")
        self.J = np.pad(nxt.astype(np.int64), pad, mode="reflect")
        ix, iy = scharr_deriv(prev)
        self.Ix = np.pad(ix, pad, mode="constant")
        self.Iy = np.pad(iy, pad, mode="constant")
        self.ww, self.wh = ww, wh

    def sample(self, plane, ix, iy, w4, shift):
        """the ww x wh window of bilinear samples whose top-left neighbour pixel is (ix, iy)"""
        y0, x0 = iy + self.wh, ix + self.ww
        win = lambda dy, dx: plane[y0 + dy:y0 + dy + self.wh, x0 + dx:x0 + dx + self.ww]
        return descale(win(0, 0) * w4[0] + win(0, 1) * w4[1] + win(1, 0) * w4[2] + win(1, 1) * w4[3], shift)

    def in_range(self, fx, fy):
        """cv2's test on the floored floats: ix >= -ww, ix < cols, iy >= -wh, iy < rows (false for anything not finite)"""
        return bool(fx >= -self.ww and fx < self.cols and fy >= -self.wh and fy < self.rows)


def _bad(v):
    return not (np.isfinite(v) and abs(float(v)) <= COORD_LIMIT)


def lk_restate(prev, nxt, pts, next_pts=None, win=(21, 21), max_level=3, max_count=30, eps=0.01, flags=0, min_eig_threshold=1e-4, info=None):
    """(nextPts (N, 2) float32, status (N,) uint8, err (N,) float32).  info (a dict): receives 'levels' and 'iters', the iterations
    every point made at level 0."""
    prev, nxt = np.asarray(prev), np.asarray(nxt)
    assert prev.dtype == np.uint8 and prev.ndim == 2 and prev.shape == nxt.shape and nxt.dtype == np.uint8
    ww, wh = int(win[0]), int(win[1])
    assert 3 <= ww <= 63 and 3 <= wh <= 63 and 0 <= max_level <= 15 and not flags & ~12
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    guess = None
    if flags & OPTFLOW_USE_INITIAL_FLOW:
        guess = np.asarray(next_pts, np.float32).reshape(-1, 2)
        assert guess.shape == pts.shape
    max_count = min(max(int(max_count), 0), 100)
    eps = min(max(float(eps), 0.0), 10.0)
    eps2 = eps * eps
    pl, nl = build_levels(prev, ww, wh, max_level), build_levels(nxt, ww, wh, max_level)
    levels = [_Level(p, q, ww, wh) for p, q in zip(pl, nl)]
    half = (f32(ww - 1) * f32(0.5), f32(wh - 1) * f32(0.5))
    area2 = float(2 * ww * wh)
    n = len(pts)
    out, status, err = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8), np.zeros(n, np.float32)
    iters = np.zeros(n, np.int32)
    with np.errstate(all="ignore"):
        for k in range(n):
            start = guess[k] if guess is not None else pts[k]
            if any(_bad(v) for v in pts[k]) or any(_bad(v) for v in start):
                out[k] = start
                continue
            ok, e, cur = 1, f32(0), None
            for lv in range(len(levels) - 1, -1, -1):
                L = levels[lv]
                scale = f32(1.0 / (1 << lv))
                px, py = pts[k][0] * scale, pts[k][1] * scale
                if lv == len(levels) - 1:
                    nx, ny = (guess[k][0] * scale, guess[k][1] * scale) if guess is not None else (px, py)
                else:
                    nx, ny = cur[0] * f32(2), cur[1] * f32(2)
                cur = [nx, ny]
                px, py = px - half[0], py - half[1]
                fx, fy = np.floor(px), np.floor(py)
                if not L.in_range(fx, fy):
                    if lv == 0:
                        ok, e = 0, f32(0)
                    continue
                ix, iy = int(fx), int(fy)
                w4 = weights(px - fx, py - fy)
                Iw = L.sample(L.I, ix, iy, w4, W_BITS - 5)
                Ixw = L.sample(L.Ix, ix, iy, w4, W_BITS)
                Iyw = L.sample(L.Iy, ix, iy, w4, W_BITS)
                A11, A12, A22 = (float(int(v)) * 2.0 ** -20 for v in ((Ixw * Ixw).sum(), (Ixw * Iyw).sum(), (Iyw * Iyw).sum()))
                D = np.float64(A11) * A22 - np.float64(A12) * A12
                dd = np.float64(A11) - A22
                min_eig = f32(((np.float64(A22) + A11) - np.sqrt(dd * dd + 4.0 * (np.float64(A12) * A12))) / area2)
                if flags & OPTFLOW_LK_GET_MIN_EIGENVALS and lv == 0:
                    e = min_eig
                if float(min_eig) < min_eig_threshold or D < FLT_EPSILON:
                    if lv == 0:
                        ok = 0
                    continue
                nx, ny = nx - half[0], ny - half[1]
                pdx = pdy = f32(0)
                for j in range(max_count):
                    fx, fy = np.floor(nx), np.floor(ny)
                    if not L.in_range(fx, fy):
                        if lv == 0:
                            ok = 0
                        break
                    if lv == 0:
                        iters[k] = j + 1
                    diff = L.sample(L.J, int(fx), int(fy), weights(nx - fx, ny - fy), W_BITS - 5) - Iw
                    b1, b2 = float(int((diff * Ixw).sum())) * 2.0 ** -20, float(int((diff * Iyw).sum())) * 2.0 ** -20
                    dx = f32((np.float64(A12) * b2 - np.float64(A22) * b1) / D)
                    dy = f32((np.float64(A12) * b1 - np.float64(A11) * b2) / D)
                    nx, ny = nx + dx, ny + dy
                    cur = [nx + half[0], ny + half[1]]
                    if np.float64(dx) * np.float64(dx) + np.float64(dy) * np.float64(dy) <= eps2:
                        break
                    if j > 0 and abs(float(dx + pdx)) < 0.01 and abs(float(dy + pdy)) < 0.01:
                        cur = [cur[0] - dx * f32(0.5), cur[1] - dy * f32(0.5)]
                        break
                    pdx, pdy = dx, dy
                if ok and lv == 0 and not flags & OPTFLOW_LK_GET_MIN_EIGENVALS:
                    ex, ey = cur[0] - half[0], cur[1] - half[1]
                    fx, fy = np.floor(ex), np.floor(ey)
                    if not L.in_range(fx, fy):
                        ok = 0
                    else:
                        diff = L.sample(L.J, int(fx), int(fy), weights(ex - fx, ey - fy), W_BITS - 5) - Iw
                        e = f32(float(int(np.abs(diff).sum())) / float(32 * ww * wh))
            out[k] = cur
            status[k] = ok
            err[k] = e if (ok or flags & OPTFLOW_LK_GET_MIN_EIGENVALS) else f32(0)
    if info is not None:
        info["levels"], info["iters"] = len(levels), iters
    return out, status, err
