"""cv2.HoughCircles(image, HOUGH_GRADIENT, dp, minDist, None, param1, param2, minRadius, maxRadius) of OpenCV 4.x (imgproc/src/hough.cpp
HoughCircles -> HoughCirclesGradient with maxRadius >= 0) restated in numpy, step by step - the statement the GPU kernels
(csrc/vp_hough_circles.hip) are held to bit for bit.

Floats are float32 wherever the C++ code uses float: every product, sum, quotient and square root of float32 numpy values is rounded on
its own (no fused multiply-add); cvRound is np.rint (half to even); integer shifts are arithmetic.  Where C loops over bins or
candidates, this file loops too.  The edges are those of cv2.Canny (the oracle's, compared with a live cv2 elsewhere), the derivatives
the 3x3 CV_16S Sobel with BORDER_REPLICATE.  The product never imports this file."""
import bisect

import numpy as np

SHIFT, ONE = 10, 1 << 10
NBINS_PER_DR = 10
F32 = np.float32
FLT_EPSILON = F32(np.finfo(np.float32).eps)


class ArgumentError(ValueError):
    """What OpenCV reports as StsOutOfRange / an assertion before any work."""


def arguments(shape, dp, min_dist, param1=100, param2=100, min_radius=0, max_radius=0):
    """Step 1: the checks and defaults of HoughCircles -> dict(dp, idp, min_dist, canny_low, canny_high, acc_thresh, min_radius,
    max_radius).  Raises ArgumentError where OpenCV raises; NotImplementedError for the centres-only mode (max_radius < 0)."""
    rows, cols = int(shape[0]), int(shape[1])
    if rows <= 0 or cols <= 0:
        raise ArgumentError("empty image")
    if not (dp > 0 and min_dist > 0 and param1 > 0 and param2 > 0):
        raise ArgumentError("dp, min_dist, canny_threshold and acc_threshold must be all positive numbers")
    canny_thresh, acc_thresh = int(np.rint(float(param1))), int(np.rint(float(param2)))    # cvRound(double): half to even
    min_radius = max(0, int(min_radius))
    max_radius = int(max_radius)
    if max_radius < 0:
        raise NotImplementedError("centres-only mode (maxRadius < 0)")
    if max_radius == 0:
        max_radius = max(rows, cols)
    elif max_radius <= min_radius:
        max_radius = min_radius + 2
    dpf = max(F32(dp), F32(1))
    return dict(dp=dpf, idp=F32(1) / dpf, min_dist=F32(min_dist), canny_low=max(1, canny_thresh // 2), canny_high=canny_thresh,
                acc_thresh=acc_thresh, min_radius=min_radius, max_radius=max_radius)


def sobel(img):
    """3x3 Sobel dx, dy (int32) of a uint8 image with BORDER_REPLICATE."""
    a = np.pad(np.asarray(img, np.int32), 1, mode="edge")
    dx = (a[:-2, 2:] + 2 * a[1:-1, 2:] + a[2:, 2:]) - (a[:-2, :-2] + 2 * a[1:-1, :-2] + a[2:, :-2])
    dy = (a[2:, :-2] + 2 * a[2:, 1:-1] + a[2:, 2:]) - (a[:-2, :-2] + 2 * a[:-2, 1:-1] + a[:-2, 2:])
    return dx, dy


def accum_size(shape, idp):
    """(arows, acols) = (cvCeil(rows * idp), cvCeil(cols * idp)), float products."""
    return int(np.ceil(F32(shape[0]) * idp)), int(np.ceil(F32(shape[1]) * idp))


def points(edges, dx, dy):
    """The point set of step 3, in raster order: (xs, ys, sx, sy, x0, y0) for every edge pixel with a non-zero gradient (mag >= 1)."""
    ys, xs = np.nonzero(edges)
    vx, vy = dx[ys, xs].astype(np.float32), dy[ys, xs].astype(np.float32)
    keep = (vx != 0) | (vy != 0)
    ys, xs, vx, vy = ys[keep], xs[keep], vx[keep], vy[keep]
    mag = np.sqrt(vx * vx + vy * vy)
    keep = mag >= F32(1)
    ys, xs, vx, vy, mag = ys[keep], xs[keep], vx[keep], vy[keep], mag[keep]
    return xs, ys, mag, vx, vy


def ray_params(xs, ys, vx, vy, mag, idp):
    sx = np.rint(((vx * idp) * F32(ONE)) / mag).astype(np.int64)
    sy = np.rint(((vy * idp) * F32(ONE)) / mag).astype(np.int64)
    x0 = np.rint((xs.astype(np.float32) * idp) * F32(ONE)).astype(np.int64)
    y0 = np.rint((ys.astype(np.float32) * idp) * F32(ONE)).astype(np.int64)
    return sx, sy, x0, y0


def vote(acc, acols, arows, sx, sy, x0, y0, min_radius, max_radius):
    """HoughCirclesAccumInvoker's rays, literally: for each sign, r = minRadius .. maxRadius, stop at the first cell outside
    [0, acols) x [0, arows), else one vote at bordered cell (y2 + 1, x2 + 1).  acc: flat int64 (arows + 2) * (acols + 2)."""
    if max_radius < min_radius or len(sx) == 0:
        return acc
    r = np.arange(min_radius, max_radius + 1, dtype=np.int64)
    step = max(1, (1 << 22) // len(r))
    for sign in (1, -1):
        for p0 in range(0, len(sx), step):
            sl = slice(p0, p0 + step)
            x1 = x0[sl, None] + r[None, :] * (sign * sx[sl, None])
            y1 = y0[sl, None] + r[None, :] * (sign * sy[sl, None])
            x2, y2 = x1 >> SHIFT, y1 >> SHIFT
            inside = (x2 >= 0) & (x2 < acols) & (y2 >= 0) & (y2 < arows)
            run = np.logical_and.accumulate(inside, axis=1)          # the `break` at the first outside cell
            idx = (y2[run] + 1) * (acols + 2) + (x2[run] + 1)
            acc += np.bincount(idx, minlength=acc.size)
    return acc


def edges_and_derivatives(img, a, canny):
    edges = canny(img, a["canny_low"], a["canny_high"])
    dx, dy = sobel(img)
    return edges, dx, dy


def accumulator(img, a, canny):
    """Steps 2-3: the (arows + 2) x (acols + 2) int64 votes (OpenCV: int32) and the point list (xs, ys)."""
    edges, dx, dy = edges_and_derivatives(img, a, canny)
    arows, acols = accum_size(img.shape, a["idp"])
    xs, ys, mag, vx, vy = points(edges, dx, dy)
    sx, sy, x0, y0 = ray_params(xs, ys, vx, vy, mag, a["idp"])
    acc = np.zeros((arows + 2) * (acols + 2), np.int64)
    vote(acc, acols, arows, sx, sy, x0, y0, a["min_radius"], a["max_radius"])
    return acc.reshape(arows + 2, acols + 2), (xs, ys)


def centres(acc, acc_thresh):
    """Step 4: bordered offsets of the centre cells, sorted by votes descending then offset ascending (hough_cmp_gt)."""
    c = acc[1:-1, 1:-1]
    m = (c > acc_thresh) & (c > acc[1:-1, :-2]) & (c >= acc[1:-1, 2:]) & (c > acc[:-2, 1:-1]) & (c >= acc[2:, 1:-1])
    y, x = np.nonzero(m)
    ofs = (y + 1) * acc.shape[1] + (x + 1)
    votes = c[y, x]
    order = np.lexsort((ofs, -votes))
    return ofs[order].astype(np.int64), votes[order]


def n_bins(a):
    return int(np.rint(F32(a["max_radius"] - a["min_radius"]) / a["dp"] * F32(NBINS_PER_DR)))


def walk_bins(bins, min_radius, dp):
    """The bin-group walk of HoughCircleEstimateRadiusInvoker, literally (j from nBins - 1 down to 1; a non-empty bin opens a group of up
    to ten bins; the for loop's own j-- follows the group's inner loop) -> (maxCount, rBest)."""
    nb = len(bins)
    nz = np.flatnonzero(bins).tolist()
    cs = np.concatenate(([0], np.cumsum(bins))).tolist()
    max_count, r_best = 0, F32(0)
    j = nb - 1
    while j > 0:
        k = bisect.bisect_right(nz, j) - 1                          # the empty bins the C loop steps over
        if k < 0 or nz[k] <= 0:
            break
        upbin = nz[k]
        j = max(upbin - NBINS_PER_DR, -1)                           # the inner loop: bins upbin down to j + 1 (at least bin 0)
        cur = cs[upbin + 1] - cs[j + 1]
        r_cur = F32(F32(upbin + j) / F32(2)) / F32(NBINS_PER_DR) * dp + F32(min_radius)
        if F32(cur) * r_best >= F32(max_count) * r_cur or (r_best < FLT_EPSILON and cur >= max_count):
            r_best, max_count = r_cur, cur
        j -= 1                                                      # the outer for loop's decrement
    return max_count, r_best


def distances(cx, cy, xs, ys, a):
    """The point-list filter: sqrt(r2) of every point with minRadius^2 <= r2 <= maxRadius^2, float32."""
    dx = cx - xs.astype(np.float32)
    dy = cy - ys.astype(np.float32)
    r2 = dx * dx + dy * dy
    min_r2 = F32(a["min_radius"]) * F32(a["min_radius"])
    max_r2 = F32(a["max_radius"]) * F32(a["max_radius"])
    return np.sqrt(r2[(min_r2 <= r2) & (r2 <= max_r2)])


def histogram(d, a, nb):
    b = np.rint((d - F32(a["min_radius"])) / a["dp"] * F32(NBINS_PER_DR)).astype(np.int64)
    return np.bincount(np.clip(b, 0, nb - 1), minlength=nb)


def estimates(ofs, acols, xs, ys, a):
    """Step 5: [(cx, cy, r, support)] in centre order, only those with support > accThresh.  Centres are taken in batches (the same
    element-wise float32 operations as distances() and histogram(), one row per centre)."""
    nb = n_bins(a)
    out = []
    if nb <= 0 or len(ofs) == 0:
        return out
    dp = a["dp"]
    y, x = np.divmod(np.asarray(ofs, np.int64), acols + 2)
    cxs = (x.astype(np.float32) + F32(0.5)) * dp
    cys = (y.astype(np.float32) + F32(0.5)) * dp
    px, py = xs.astype(np.float32), ys.astype(np.float32)
    min_r2 = F32(a["min_radius"]) * F32(a["min_radius"])
    max_r2 = F32(a["max_radius"]) * F32(a["max_radius"])
    step = max(1, (1 << 22) // max(1, len(px)))
    for c0 in range(0, len(cxs), step):
        cx, cy = cxs[c0:c0 + step], cys[c0:c0 + step]
        dx = cx[:, None] - px[None, :]
        dy = cy[:, None] - py[None, :]
        r2 = dx * dx + dy * dy
        keep = (min_r2 <= r2) & (r2 <= max_r2)
        rows, cols = np.nonzero(keep)
        d = np.sqrt(r2[rows, cols])
        b = np.clip(np.rint((d - F32(a["min_radius"])) / dp * F32(NBINS_PER_DR)).astype(np.int64), 0, nb - 1)
        for k in range(len(cx)):
            sel = b[np.searchsorted(rows, k):np.searchsorted(rows, k, side="right")]
            max_count, r_best = walk_bins(np.bincount(sel, minlength=nb), a["min_radius"], dp) if sel.size else (0, F32(0))
            if max_count > a["acc_thresh"]:
                out.append((cx[k], cy[k], r_best, max_count))
    return out


def order(est):
    """Step 6 (cmpAccum): support descending, r descending, x ascending, y ascending."""
    return sorted(est, key=lambda e: (-e[3], -float(e[2]), float(e[0]), float(e[1])))


def remove_overlaps(circles, min_dist):
    """Step 7 (RemoveOverlaps / CheckDistance): greedy, the first kept; a later one kept when no kept one lies closer than minDist
    (dx * dx + dy * dy < minDist^2 in float32; the kept ones are checked all at once, which gives the same verdict as C's early exit)."""
    if len(circles) <= 1:
        return list(circles)
    md2 = F32(min_dist) * F32(min_dist)
    kept = [circles[0]]
    kx, ky = np.empty(len(circles), np.float32), np.empty(len(circles), np.float32)
    kx[0], ky[0] = circles[0][0], circles[0][1]
    for c in circles[1:]:
        n = len(kept)
        ddx, ddy = F32(c[0]) - kx[:n], F32(c[1]) - ky[:n]
        if not np.any(ddx * ddx + ddy * ddy < md2):
            kx[n], ky[n] = c[0], c[1]
            kept.append(c)
    return kept


def hough_circles(img, dp, min_dist, param1=100, param2=100, min_radius=0, max_radius=0, canny=None):
    """cv2.HoughCircles(img, HOUGH_GRADIENT, dp, min_dist, None, param1, param2, min_radius, max_radius): (1, N, 3) float32 or None.
    canny(img, low, high): the edge detector (the oracle's cv2.Canny by default)."""
    if canny is None:
        from oracle import oracle as orc
        canny = orc.canny
    img = np.ascontiguousarray(img)
    a = arguments(img.shape, dp, min_dist, param1, param2, min_radius, max_radius)
    acc, (xs, ys) = accumulator(img, a, canny)
    if len(xs) == 0:
        return None
    ofs, _ = centres(acc, a["acc_thresh"])
    kept = remove_overlaps(order(estimates(ofs, acc.shape[1] - 2, xs, ys, a)), a["min_dist"])
    if not kept:
        return None
    return np.array([[(c[0], c[1], c[2]) for c in kept]], np.float32)
