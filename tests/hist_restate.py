"""The numpy statement of the colour-histogram family: what vp_calc_hist_*, vp_back_project_* and
vp_mean_shift_dev compute, and the finishing arithmetic of CamShift.  It follows OpenCV's calcHistLookupTables_8u / calcHist_8u,
calcBackProj_8u, meanShift and CamShift step by step, uses nothing of the library under test, and is itself checked by hand in
tests/test_hist_statement.py.  Windows are (x, y, w, h)."""
import math

import numpy as np

DBL_EPSILON = 2.220446049250313e-16
TOLERANCE = 10


def round_half_even(v):
    return int(np.rint(np.float64(v)))


def bin_tables(hist_size, ranges):
    """per dimension the bin of every byte value, -1 where it falls into none: a = size / (high - low), b = -a * low in double,
    bin(j) = floor(j * a + b), kept when 0 <= bin < size (the upper end of a range is exclusive)"""
    tabs = []
    for size, (lo, hi) in zip(hist_size, np.asarray(ranges, np.float64).reshape(-1, 2)):
        a = np.float64(size) / (np.float64(hi) - np.float64(lo))
        b = -a * np.float64(lo)
        t = np.full(256, -1, np.int64)
        for j in range(256):
            idx = int(math.floor(np.float64(j) * a + b))
            if 0 <= idx < size:
                t[j] = idx
        tabs.append(t)
    return tabs


def _channels(img):
    return img.reshape(img.shape[0], img.shape[1], -1)


def pixel_bins(img, channels, hist_size, ranges):
    """the flat bin of every pixel (first dimension slowest), -1 for a pixel without one"""
    px = _channels(img)
    tabs = bin_tables(hist_size, ranges)
    flat = np.zeros(px.shape[:2], np.int64)
    out = np.zeros(px.shape[:2], bool)
    for c, size, t in zip(channels, hist_size, tabs):
        b = t[px[:, :, c]]
        out |= b < 0
        flat = flat * size + np.where(b < 0, 0, b)
    return np.where(out, -1, flat)


def calc_hist_counts(img, channels, hist_size, ranges, mask=None):
    """exact counts, uint32, shape hist_size: the counting loop"""
    bins = pixel_bins(img, channels, hist_size, ranges)
    take = bins >= 0
    if mask is not None:
        take &= np.asarray(mask) != 0
    total = int(np.prod(hist_size))
    return np.bincount(bins[take], minlength=total).astype(np.uint32).reshape(tuple(hist_size))


def calc_hist(img, channels, hist_size, ranges, mask=None):
    return calc_hist_counts(img, channels, hist_size, ranges, mask).astype(np.float32)


def fold(hist, scale):
    """one byte per bin: saturate_u8(round_half_even(double(hist) * scale)); a NaN gives 0"""
    out = np.zeros(hist.size, np.uint8)
    for i, v in enumerate(np.asarray(hist, np.float32).reshape(-1)):
        p = np.float64(v) * np.float64(scale)
        if p != p:
            continue
        r = np.rint(p)
        out[i] = 0 if r <= 0 else 255 if r >= 255 else int(r)
    return out.reshape(np.shape(hist))


def back_project(img, channels, hist, ranges, scale):
    bins = pixel_bins(img, channels, np.shape(hist), ranges)
    table = np.concatenate([fold(hist, scale).reshape(-1), np.zeros(1, np.uint8)])
    return table[bins]                      # -1 reads the zero at the end


def normalize_hist(hist, top=255.0, low=0.0):
    """the library's min-max stretch: in double, rounded once"""
    v = np.asarray(hist, np.float32).astype(np.float64)
    lo, hi = v.min(), v.max()
    if not hi > lo:
        return np.full(v.shape, low, np.float32)
    return (np.float64(low) + (v - lo) * ((np.float64(top) - np.float64(low)) / (hi - lo))).astype(np.float32)


def intersect(win, cols, rows):
    """cv2's Rect & Rect(0, 0, cols, rows): the empty Rect() is (0, 0, 0, 0)"""
    x, y, w, h = win
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, cols), min(y + h, rows)
    return (x0, y0, x1 - x0, y1 - y0) if x1 > x0 and y1 > y0 else (0, 0, 0, 0)


def window_sums(prob, cur):
    """m00, m10, m01 of the window as Python integers, x and y relative to its corner"""
    x, y, w, h = cur
    p = prob[y:y + h, x:x + w].astype(object)
    return int(p.sum()), int((p * np.arange(w, dtype=object)[None, :]).sum()), int((p * np.arange(h, dtype=object)[:, None]).sum())


def window_sums_fast(prob, cur):
    """the same integers through int64 row and column sums (exact: a first moment stays below 2^53)"""
    x, y, w, h = cur
    p = prob[y:y + h, x:x + w].astype(np.int64)
    cols, rows = p.sum(axis=0), p.sum(axis=1)
    return int(cols.sum()), int((cols * np.arange(w, dtype=np.int64)).sum()), int((rows * np.arange(h, dtype=np.int64)).sum())


def criteria(max_iter=None, eps=None):
    """(niters, eps2) of cv2's meanShift: no MAX_ITER criterion (None) is 100 iterations, no EPS criterion is eps2 = 1"""
    niters = 100 if max_iter is None else max(int(max_iter), 1)
    eps2 = 1 if eps is None else round_half_even(max(float(eps), 0.0) ** 2)
    return niters, eps2


def mean_shift_loop(prob, start, W, niters, eps2, sums=window_sums_fast):
    """the loop from a current window `start` with the size of W for the step: ((x, y, w, h), i)"""
    rows, cols = prob.shape
    cur = tuple(start)
    i = 0
    while i < niters:
        cur = intersect(cur, cols, rows)
        if cur == (0, 0, 0, 0):
            cur = (cols // 2, rows // 2, 0, 0)
        cur = (cur[0], cur[1], max(cur[2], 1), max(cur[3], 1))
        m00, m10, m01 = sums(prob, cur)
        if m00 == 0:
            break
        dx = round_half_even(np.float64(m10) / np.float64(m00) - np.float64(W[2]) * 0.5)
        dy = round_half_even(np.float64(m01) / np.float64(m00) - np.float64(W[3]) * 0.5)
        nx = min(max(cur[0] + dx, 0), cols - cur[2])
        ny = min(max(cur[1] + dy, 0), rows - cur[3])
        dx, dy = nx - cur[0], ny - cur[1]
        cur = (nx, ny, cur[2], cur[3])
        if dx * dx + dy * dy < eps2:
            break
        i += 1
    return cur, i


def mean_shift(prob, window, max_iter=None, eps=None):
    """(iterations, window); a window of non-positive size, or with nothing of it inside the image, is refused (ValueError)"""
    rows, cols = prob.shape
    if window[2] <= 0 or window[3] <= 0:
        raise ValueError("non-positive size")
    W = intersect(tuple(int(v) for v in window), cols, rows)
    if W == (0, 0, 0, 0):
        raise ValueError("empty inside the image")
    niters, eps2 = criteria(max_iter, eps)
    cur, i = mean_shift_loop(prob, W, W, niters, eps2)
    return i, cur


def raster_sums(prob, win):
    """m00 m10 m01 m20 m11 m02 of the window as Python integers"""
    x, y, w, h = win
    p = prob[y:y + h, x:x + w].astype(object)
    xs, ys = np.arange(w, dtype=object)[None, :], np.arange(h, dtype=object)[:, None]
    return tuple(int(v) for v in (p.sum(), (p * xs).sum(), (p * ys).sum(), (p * xs * xs).sum(), (p * xs * ys).sum(), (p * ys * ys).sum()))


def grow(win, cols, rows):
    x, y, w, h = win
    x, y = max(x - TOLERANCE, 0), max(y - TOLERANCE, 0)
    w, h = w + 2 * TOLERANCE, h + 2 * TOLERANCE
    if x + w > cols:
        w = cols - x
    if y + h > rows:
        h = rows - y
    return x, y, w, h


def cam_shift_finish(sums, window, cols, rows):
    """cv2's CamShift after the moments of the grown window: (((cx, cy), (w, h), angle), window), evaluated with this host's libm"""
    m00, m10, m01, m20, m11, m02 = (float(s) for s in sums)
    x, y, w, h = window
    if abs(m00) < DBL_EPSILON:
        return ((0.0, 0.0), (0.0, 0.0), 0.0), window
    inv_m00 = 1.0 / m00
    cx, cy = m10 * inv_m00, m01 * inv_m00                           # completeMomentState
    mu20, mu11, mu02 = m20 - m10 * cx, m11 - m10 * cy, m02 - m01 * cy
    xc = round_half_even(m10 * inv_m00 + x)
    yc = round_half_even(m01 * inv_m00 + y)
    a, b, c = mu20 * inv_m00, mu11 * inv_m00, mu02 * inv_m00
    square = math.sqrt(4 * b * b + (a - c) * (a - c))
    theta = math.atan2(2 * b, a - c + square)
    cs, sn = math.cos(theta), math.sin(theta)
    rotate_a = cs * cs * mu20 + 2 * cs * sn * mu11 + sn * sn * mu02
    rotate_c = sn * sn * mu20 - 2 * cs * sn * mu11 + cs * cs * mu02
    rotate_a, rotate_c = max(0.0, rotate_a), max(0.0, rotate_c)
    length = math.sqrt(rotate_a * inv_m00) * 4
    width = math.sqrt(rotate_c * inv_m00) * 4
    if length < width:
        length, width = width, length
        cs, sn = sn, cs
        theta = math.pi * 0.5 - theta
    t0 = max(round_half_even(abs(length * cs)), round_half_even(abs(width * sn))) + 2
    w = min(t0, (cols - xc) * 2)
    t0 = max(round_half_even(abs(length * sn)), round_half_even(abs(width * cs))) + 2
    h = min(t0, (rows - yc) * 2)
    x = max(0, xc - int(w / 2))
    y = max(0, yc - int(h / 2))
    w = min(cols - x, w)
    h = min(rows - y, h)
    angle = np.float32((math.pi * 0.5 + theta) * 180.0 / math.pi)
    while angle < 0:
        angle = np.float32(angle + np.float32(360))
    while angle >= 360:
        angle = np.float32(angle - np.float32(360))
    if angle >= 180:
        angle = np.float32(angle - np.float32(180))
    centre = (float(np.float32(x) + np.float32(w) * np.float32(0.5)), float(np.float32(y) + np.float32(h) * np.float32(0.5)))
    return (centre, (float(np.float32(width)), float(np.float32(length))), float(angle)), (x, y, w, h)


def cam_shift(prob, window, max_iter=None, eps=None):
    rows, cols = prob.shape
    _, found = mean_shift(prob, window, max_iter, eps)
    grown = grow(found, cols, rows)
    return cam_shift_finish(raster_sums(prob, grown), grown, cols, rows)
