"""The statement of stereo block matching, in numpy: what vp_stereo_bm_* and vp_depth_from_disparity_* must equal
byte for byte.  It follows the design of OpenCV's StereoBM step by step - XSOBEL prefilter, SAD over a square window, texture and
uniqueness tests, parabola subpixel - and where the text below fixes a rule, the rule is the contract: it has not met a real OpenCV.

  prefilter   rows reflected without the edge row (row -1 is row 1, row h is row h - 2; a single row is its own neighbour):
              p = clamp(I(x+1,y-1) - I(x-1,y-1) + 2 (I(x+1,y) - I(x-1,y)) + I(x+1,y+1) - I(x-1,y+1), -c, c) + c for 1 <= x <= w - 2;
              columns 0 and w - 1 are c
  cost        C(x, y, D) = sum over |i|, |j| <= r of |pL(x+i, y+j) - pR(x+i-D, y+j)|, D in [m, m + n - 1]
  candidates  r <= y <= h-1-r, r <= x <= w-1-r, x - r - (m+n-1) >= 0, x + r - m <= w - 1; everything else is INV = (m - 1) * 16
  texture     T = window sum of |pL - c|; T < texture_threshold gives INV
  best        D* minimises C, ties to the larger D
  uniqueness  (ratio > 0 only) t = C* + C* ratio // 100; any D with |D - D*| > 1 and C(D) <= t gives INV
  subpixel    pm = C(D*-1), pp = C(D*+1), the one missing at an end of the range is the other; den = pm + pp - 2 C* + |pm - pp|;
              off = 0 if den == 0 else (pm - pp) 256 / den truncated; int16 (D* 256 + off + 15) >> 4
  depth       float32(float64(focal_px * baseline_m) * 16.0 / float64(disp16)) for disp16 > 0, else 0
"""
import numpy as np

DEFAULTS = dict(num_disparities=64, block_size=15, min_disparity=0, pre_filter_cap=31, texture_threshold=10, uniqueness_ratio=15)


def invalid_disparity(min_disparity=0):
    return (int(min_disparity) - 1) * 16


def valid_rect(w, h, num_disparities=64, block_size=15, min_disparity=0):
    """(x, y, w, h) of the candidate pixels; (0, 0, 0, 0) when there is none"""
    r, m, n = block_size // 2, min_disparity, num_disparities
    x0 = max(r, r + m + n - 1)
    x1 = min(w - 1 - r, w - 1 - r + m)
    y0, y1 = r, h - 1 - r
    if x1 < x0 or y1 < y0:
        return (0, 0, 0, 0)
    return (x0, y0, x1 - x0 + 1, y1 - y0 + 1)


def prefilter(img, cap):
    img = np.asarray(img).astype(np.int32)
    h, w = img.shape
    out = np.full((h, w), cap, np.int32)
    if w >= 3:
        rows = np.pad(img, ((1, 1), (0, 0)), mode="reflect" if h > 1 else "edge")
        dx = rows[:, 2:] - rows[:, :-2]
        s = dx[:-2] + 2 * dx[1:-1] + dx[2:]
        out[:, 1:-1] = np.clip(s, -cap, cap) + cap
    return out


def _box(a, r):
    """sums over (2r+1) x (2r+1) windows that lie inside a: shape (h - 2r, w - 2r)"""
    k = 2 * r + 1
    s = np.zeros((a.shape[0] + 1, a.shape[1] + 1), np.int64)
    s[1:, 1:] = a.cumsum(0).cumsum(1)
    return s[k:, k:] - s[:-k, k:] - s[k:, :-k] + s[:-k, :-k]


def cost_volume(left, right, num_disparities, block_size, min_disparity, pre_filter_cap):
    """(C of shape (n, ch, cw), T of shape (ch, cw), rect) over the candidate rectangle; None when it is empty"""
    h, w = np.asarray(left).shape
    n, m, r = num_disparities, min_disparity, block_size // 2
    x0, y0, cw, ch = valid_rect(w, h, n, block_size, m)
    if cw == 0:
        return None
    pl, pr = prefilter(left, pre_filter_cap), prefilter(right, pre_filter_cap)
    a, b = x0 - r, x0 + cw + r                       # the columns of left under the windows of the candidates
    C = np.empty((n, ch, cw), np.int32)
    for d in range(n):
        D = m + d
        C[d] = _box(np.abs(pl[:, a:b] - pr[:, a - D:b - D]), r)
    T = _box(np.abs(pl[:, a:b] - pre_filter_cap), r).astype(np.int32)
    return C, T, (x0, y0, cw, ch)


def disparity(left, right, num_disparities=64, block_size=15, min_disparity=0, pre_filter_cap=31, texture_threshold=10, uniqueness_ratio=15):
    left, right = np.asarray(left), np.asarray(right)
    assert left.dtype == np.uint8 and right.dtype == np.uint8 and left.ndim == 2 and left.shape == right.shape
    n, m = int(num_disparities), int(min_disparity)
    assert 16 <= n <= 256 and n % 16 == 0 and block_size % 2 == 1 and 5 <= block_size <= 21 and -128 <= m <= 128
    assert 1 <= pre_filter_cap <= 63 and texture_threshold >= 0 and 0 <= uniqueness_ratio <= 100
    h, w = left.shape
    out = np.full((h, w), invalid_disparity(m), np.int16)
    cv = cost_volume(left, right, n, block_size, m, pre_filter_cap)
    if cv is None:
        return out
    C, T, (x0, y0, cw, ch) = cv
    ds = n - 1 - np.argmin(C[::-1], axis=0)                                   # the last minimum: ties to the larger D
    take = lambda d: np.take_along_axis(C, d[None], axis=0)[0]
    cmin = take(ds)
    keep = T >= texture_threshold
    if uniqueness_ratio > 0:
        limit = cmin + cmin * uniqueness_ratio // 100
        far = np.abs(np.arange(n)[:, None, None] - ds[None]) > 1
        keep &= ~np.any(far & (C <= limit[None]), axis=0)
    pm = take(np.where(ds > 0, ds - 1, ds + 1))
    pp = take(np.where(ds < n - 1, ds + 1, ds - 1))
    num = (pm - pp).astype(np.int64) * 256
    den = (pm + pp - 2 * cmin + np.abs(pm - pp)).astype(np.int64)
    off = np.where(den == 0, 0, np.sign(num) * (np.abs(num) // np.maximum(den, 1)))   # C's division: towards zero
    val = ((m + ds).astype(np.int64) * 256 + off + 15) >> 4
    out[y0:y0 + ch, x0:x0 + cw] = np.where(keep, val, invalid_disparity(m)).astype(np.int16)
    return out


def depth_from_disparity(disp16, focal_px, baseline_m):
    disp16 = np.asarray(disp16)
    assert disp16.dtype == np.int16
    fb = np.float64(float(focal_px) * float(baseline_m))
    d = disp16.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (fb * 16.0 / d).astype(np.float32)
    return np.where(disp16 > 0, z, np.float32(0)).astype(np.float32)
