"""The statement of robust motion estimation from point pairs as this library defines it, in Python and
numpy: the oracle of tests/test_model_abi.py and tests/test_gpu_model.py.  The product never imports this file, and this file
imports nothing of the product.  The library must equal it bit for bit: model, inlier mask, inlier count, hypotheses taken.

Every floating-point value is an IEEE double (a Python float, or a numpy float64 array where the same expression is applied to
every point independently); every expression is written with explicit parentheses in the one order that counts; sums over points
are sequential in index order.

  sampling    key = mix(seed ^ (0x9e3779b9 (j + 1))), draw d: u = mix(key + d), index (u n) >> 32; lowbias32 mixer, 32-bit wrap.  Draws
              0, 1, ... until m distinct indices are collected (m = 2 similarity, 3 affine, 4 homography); void after 16 draws.
  void        a sample coordinate that is not finite; two sample points equal in either set; for m >= 3 a collinear triple in either
              set, |cross| <= FLT_EPSILON (|dx1| + |dy1| + |dx2| + |dy2|); for the homography a triple whose orientation differs
              between the sets while another's does not (cv2's checkSubset); a pivot below 1e-10; a model entry that is not finite.
  solvers     both sets are shifted by the sample's first point; similarity in closed form, affine by Cramer's rule on the two
              remaining difference vectors, homography (h33 = 1) by 8 x 8 elimination with partial pivoting (the first largest
              |pivot|); then the shift is folded back into the nine numbers.
  scoring     u = (h0 x + h1 y) + h2, v = (h3 x + h4 y) + h5, for the homography both divided by w = (h6 x + h7 y) + h8;
              err = dx dx + dy dy; inlier iff err <= threshold threshold.  The best hypothesis has the largest count, the lowest j
              among equals.  No valid hypothesis, or a best count below m: no model.
  rounds      ROUND = 256 hypotheses at a time; after round r the search stops when the best count has reached need[r], the
              smallest c in m .. n (by bisection) with cv2's RANSACUpdateNumIters(confidence, 1 - c / n, m, max_iters) <= r ROUND; at
              the latest after ceil(max_iters / ROUND) rounds, the last one cut at max_iters.
  answer      the mask is the inlier set of the best hypothesis; the model is the least-squares refit over it (refit below)."""
import math

import numpy as np

SIMILARITY, AFFINE, HOMOGRAPHY = 0, 1, 2
ROUND = 256
MAX_DRAWS = 16
COLLINEAR_EPS = 1.1920928955078125e-07
PIVOT_MIN = 1e-10
REFIT_EPS = 1e-12
DBL_MIN = 2.2250738585072014e-308
M32 = 0xFFFFFFFF


def mix(x):
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def sample(n, m, seed, j):
    """(indices padded with -1 to four, complete?)"""
    key = mix((seed ^ ((0x9E3779B9 * (j + 1)) & M32)) & M32)
    s = []
    for d in range(MAX_DRAWS):
        if len(s) == m:
            break
        idx = (mix((key + d) & M32) * n) >> 32
        if idx not in s:
            s.append(idx)
    return s + [-1] * (4 - len(s)), len(s) == m


def _collinear(ax, ay, bx, by, cx, cy):
    dx1, dy1, dx2, dy2 = bx - ax, by - ay, cx - ax, cy - ay
    cr = dx1 * dy2 - dy1 * dx2
    return cr, not (abs(cr) > COLLINEAR_EPS * (((abs(dx1) + abs(dy1)) + abs(dx2)) + abs(dy2)))


def solve8(A, b):
    """8 x 8 elimination, partial pivoting by the first largest |pivot|; None when a pivot is below PIVOT_MIN (or NaN)"""
    A = [list(r) for r in A]
    b = list(b)
    for c in range(8):
        piv, amax = c, abs(A[c][c])
        for r in range(c + 1, 8):
            if abs(A[r][c]) > amax:
                amax, piv = abs(A[r][c]), r
        if not amax >= PIVOT_MIN:
            return None
        if piv != c:
            A[c], A[piv] = A[piv], A[c]
            b[c], b[piv] = b[piv], b[c]
        for r in range(c + 1, 8):
            f = A[r][c] / A[c][c]
            for k in range(c + 1, 8):
                A[r][k] = A[r][k] - f * A[c][k]
            b[r] = b[r] - f * b[c]
    g = [0.0] * 8
    for c in range(7, -1, -1):
        s = b[c]
        for k in range(c + 1, 8):
            s = s - A[c][k] * g[k]
        g[c] = s / A[c][c]
    return g


def _div(a, b):
    """IEEE division of Python floats (no exception on a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def hypothesis(src, dst, model, seed, j):
    """(sample of four indices, nine floats or None when void)"""
    n, m = len(src), model + 2
    s, complete = sample(n, m, seed, j)
    if not complete:
        return s, None
    px = [float(src[i][0]) for i in s[:m]]
    py = [float(src[i][1]) for i in s[:m]]
    qx = [float(dst[i][0]) for i in s[:m]]
    qy = [float(dst[i][1]) for i in s[:m]]
    if not all(math.isfinite(v) for v in px + py + qx + qy):
        return s, None
    for a in range(m):
        for b in range(a + 1, m):
            if (px[a] == px[b] and py[a] == py[b]) or (qx[a] == qx[b] and qy[a] == qy[b]):
                return s, None
    det = 0.0
    if m >= 3:
        flips = 0
        for t, (a, b, c) in enumerate([(0, 1, 2)] if m == 3 else [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)]):
            cs, flat = _collinear(px[a], py[a], px[b], py[b], px[c], py[c])
            if flat:
                return s, None
            cd, flat = _collinear(qx[a], qy[a], qx[b], qy[b], qx[c], qy[c])
            if flat:
                return s, None
            if t == 0:
                det = cs
            flips += (cs < 0) != (cd < 0)
        if model == HOMOGRAPHY and flips not in (0, 4):
            return s, None
    p0x, p0y, q0x, q0y = px[0], py[0], qx[0], qy[0]
    with np.errstate(all="ignore"):
        if model == SIMILARITY:
            dx, dy, ex, ey = px[1] - p0x, py[1] - p0y, qx[1] - q0x, qy[1] - q0y
            den = dx * dx + dy * dy
            if not den > 0:
                return s, None
            c, sn = _div(dx * ex + dy * ey, den), _div(dx * ey - dy * ex, den)
            H = [c, -sn, q0x - (c * p0x - sn * p0y), sn, c, q0y - (sn * p0x + c * p0y), 0.0, 0.0, 1.0]
        elif model == AFFINE:
            a1x, a1y, a2x, a2y = px[1] - p0x, py[1] - p0y, px[2] - p0x, py[2] - p0y
            b1x, b1y, b2x, b2y = qx[1] - q0x, qy[1] - q0y, qx[2] - q0x, qy[2] - q0y
            m00, m01 = _div(b1x * a2y - b2x * a1y, det), _div(b2x * a1x - b1x * a2x, det)
            m10, m11 = _div(b1y * a2y - b2y * a1y, det), _div(b2y * a1x - b1y * a2x, det)
            H = [m00, m01, q0x - (m00 * p0x + m01 * p0y), m10, m11, q0y - (m10 * p0x + m11 * p0y), 0.0, 0.0, 1.0]
        else:
            A, b = [], []
            for k in range(4):
                x, y, X, Y = px[k] - p0x, py[k] - p0y, qx[k] - q0x, qy[k] - q0y
                A.append([x, y, 1.0, 0.0, 0.0, 0.0, -(x * X), -(y * X)])
                A.append([0.0, 0.0, 0.0, x, y, 1.0, -(x * Y), -(y * Y)])
                b += [X, Y]
            g = solve8(A, b)
            if g is None:
                return s, None
            c2, c5, c8 = g[2] - (g[0] * p0x + g[1] * p0y), g[5] - (g[3] * p0x + g[4] * p0y), 1.0 - (g[6] * p0x + g[7] * p0y)
            H = [g[0] + q0x * g[6], g[1] + q0x * g[7], c2 + q0x * c8, g[3] + q0y * g[6], g[4] + q0y * g[7], c5 + q0y * c8, g[6], g[7], c8]
    if not all(math.isfinite(v) for v in H):
        return s, None
    return s, H


def inliers(H, model, src, dst, t2):
    """bool (n,): the same expression on every point, float64"""
    x, y, X, Y = (np.asarray(a, np.float64) for a in (src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]))
    h = [np.float64(v) for v in H]
    with np.errstate(all="ignore"):
        u = (h[0] * x + h[1] * y) + h[2]
        v = (h[3] * x + h[4] * y) + h[5]
        if model == HOMOGRAPHY:
            w = (h[6] * x + h[7] * y) + h[8]
            u = u / w
            v = v / w
        dx, dy = u - X, v - Y
        return dx * dx + dy * dy <= np.float64(t2)


def num_iters(p, ep, m, max_iters):
    """cv2's RANSACUpdateNumIters"""
    p, ep = min(max(p, 0.0), 1.0), min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    denom = 1.0 - math.pow(1.0 - ep, float(m))
    if denom < DBL_MIN:
        return 0
    num, denom = math.log(num), math.log(denom)
    if denom >= 0 or -num >= max_iters * (-denom):
        return max_iters
    return round(num / denom)


def stop_table(n, model, confidence, max_iters):
    m = model + 2
    need = []
    for r in range(1, (max_iters + ROUND - 1) // ROUND + 1):
        lo, hi = m, n
        while lo < hi:
            mid = lo + (hi - lo) // 2
            if num_iters(confidence, 1.0 - mid / n, m, max_iters) <= r * ROUND:
                hi = mid
            else:
                lo = mid + 1
        need.append(lo)
    return need


def _seq(values):
    """0.0 + v0 + v1 + ... strictly in order (np.add.accumulate is sequential)"""
    return float(np.add.accumulate(np.concatenate([[0.0], np.asarray(values, np.float64)]))[-1])


def refit(src, dst, mask, model):
    """the least squares over the points whose mask byte is not 0 (None: all), nine floats or None"""
    src, dst = np.asarray(src, np.float32).reshape(-1, 2), np.asarray(dst, np.float32).reshape(-1, 2)
    keep = np.ones(len(src), bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    px, py = src[keep, 0].astype(np.float64), src[keep, 1].astype(np.float64)
    qx, qy = dst[keep, 0].astype(np.float64), dst[keep, 1].astype(np.float64)
    cnt = len(px)
    if cnt < model + 2:
        return None
    with np.errstate(all="ignore"):
        k = float(cnt)
        cpx, cpy, cqx, cqy = _div(_seq(px), k), _div(_seq(py), k), _div(_seq(qx), k), _div(_seq(qy), k)
        dx, dy, ex, ey = px - cpx, py - cpy, qx - cqx, qy - cqy
        if model == SIMILARITY:
            Sxx, Sa, Sb = _seq(dx * dx + dy * dy), _seq(dx * ex + dy * ey), _seq(dx * ey - dy * ex)
            if not Sxx > 0:
                return None
            a, b = _div(Sa, Sxx), _div(Sb, Sxx)
            H = [a, -b, cqx - (a * cpx - b * cpy), b, a, cqy - (b * cpx + a * cpy), 0.0, 0.0, 1.0]
        elif model == AFFINE:
            Sxx, Sxy, Syy = _seq(dx * dx), _seq(dx * dy), _seq(dy * dy)
            SxX, SyX, SxY, SyY = _seq(dx * ex), _seq(dy * ex), _seq(dx * ey), _seq(dy * ey)
            det = Sxx * Syy - Sxy * Sxy
            if not det > REFIT_EPS * (Sxx * Syy):
                return None
            m00, m01 = _div(SxX * Syy - SyX * Sxy, det), _div(SyX * Sxx - SxX * Sxy, det)
            m10, m11 = _div(SxY * Syy - SyY * Sxy, det), _div(SyY * Sxx - SxY * Sxy, det)
            H = [m00, m01, cqx - (m00 * cpx + m01 * cpy), m10, m11, cqy - (m10 * cpx + m11 * cpy), 0.0, 0.0, 1.0]
        else:
            apx, apy, aqx, aqy = _seq(np.abs(dx)), _seq(np.abs(dy)), _seq(np.abs(ex)), _seq(np.abs(ey))
            if not (apx > 0 and apy > 0 and aqx > 0 and aqy > 0):
                return None
            s1x, s1y, s2x, s2y = k / apx, k / apy, k / aqx, k / aqy
            x, y, X, Y = dx * s1x, dy * s1y, ex * s2x, ey * s2y
            one, zero = np.ones(cnt), np.zeros(cnt)
            r0 = [x, y, one, zero, zero, zero, -(x * X), -(y * X)]
            r1 = [zero, zero, zero, x, y, one, -(x * Y), -(y * Y)]

            def both(a, b):                     # a0, b0, a1, b1, ...: the first row's term of a point, then the second row's
                out = np.empty(2 * cnt)
                out[0::2], out[1::2] = a, b
                return out

            A = [[0.0] * 8 for _ in range(8)]
            rhs = [0.0] * 8
            for r in range(8):
                for c in range(r, 8):
                    A[r][c] = A[c][r] = _seq(both(r0[r] * r0[c], r1[r] * r1[c]))
                rhs[r] = _seq(both(r0[r] * X, r1[r] * Y))
            g = solve8(A, rhs)
            if g is None:
                return None
            e0, e1 = g[0] * s1x, g[1] * s1y
            e2 = g[2] - (e0 * cpx + e1 * cpy)
            e3, e4 = g[3] * s1x, g[4] * s1y
            e5 = g[5] - (e3 * cpx + e4 * cpy)
            e6, e7 = g[6] * s1x, g[7] * s1y
            e8 = 1.0 - (e6 * cpx + e7 * cpy)
            f = [_div(e0, s2x) + cqx * e6, _div(e1, s2x) + cqx * e7, _div(e2, s2x) + cqx * e8,
                 _div(e3, s2y) + cqy * e6, _div(e4, s2y) + cqy * e7, _div(e5, s2y) + cqy * e8, e6, e7, e8]
            if not math.isfinite(e8) or e8 == 0:
                return None
            H = [_div(v, e8) for v in f]
    if not all(math.isfinite(v) for v in H):
        return None
    return H


def estimate(src, dst, model, threshold=3.0, max_iters=2000, confidence=0.99, seed=0):
    """(nine floats or None, mask uint8 (n,), inlier count, hypotheses taken, index of the best hypothesis)"""
    src, dst = np.asarray(src, np.float32).reshape(-1, 2), np.asarray(dst, np.float32).reshape(-1, 2)
    n, m = len(src), model + 2
    t2 = threshold * threshold
    need = stop_table(n, model, confidence, max_iters)
    best, best_j, B, taken = -1, -1, None, 0
    for r in range(len(need)):
        end = min((r + 1) * ROUND, max_iters)
        for j in range(r * ROUND, end):
            _, H = hypothesis(src, dst, model, seed, j)
            if H is None:
                continue
            c = int(inliers(H, model, src, dst, t2).sum())
            if c > best:
                best, best_j, B = c, j, H
        taken = end
        if best >= need[r]:
            break
    none = (None, np.zeros(n, np.uint8), 0, taken, best_j)
    if best < m:
        return none
    mask = inliers(B, model, src, dst, t2).astype(np.uint8)
    H = refit(src, dst, mask, model)
    if H is None:
        return none
    return H, mask, int(mask.sum()), taken, best_j


def bits(H):
    """nine doubles as uint64, zeros for None: what the tests compare"""
    return np.zeros(9, np.uint64) if H is None else np.array(H, np.float64).view(np.uint64)


# ---- inputs shared by the CPU and the GPU suite -------------------------------------------------------------------------------------
def true_model(model, seed=0):
    """an exact model of a plausible frame-to-frame motion on [0, 2048)^2, 3 x 3 float64"""
    r = np.random.default_rng(1000 + 10 * seed + model)
    ang, sc = r.uniform(-0.3, 0.3), r.uniform(0.8, 1.25)
    H = np.eye(3)
    H[:2, :2] = sc * np.array([[math.cos(ang), -math.sin(ang)], [math.sin(ang), math.cos(ang)]])
    H[:2, 2] = r.uniform(-60, 60, 2)
    if model >= AFFINE:
        H[:2, :2] += r.uniform(-0.08, 0.08, (2, 2))
    if model == HOMOGRAPHY:
        H[2, :2] = r.uniform(-4e-5, 4e-5, 2)
    return H


def make_pairs(n, model, outliers, seed=0):
    """(src, dst float32 (n, 2), true inlier mask bool, the exact model): src uniform on [0, 2048)^2, dst = model(src) rounded to
    float32, the share `outliers` of the pairs (chosen at random) given a uniform random partner instead"""
    r = np.random.default_rng(77 + 1000 * seed + 31 * n + model)
    H = true_model(model, seed)
    src = r.uniform(0, 2048, (n, 2)).astype(np.float32)
    s = src.astype(np.float64)
    w = H[2, 0] * s[:, 0] + H[2, 1] * s[:, 1] + H[2, 2]
    dst = np.stack([(H[0, 0] * s[:, 0] + H[0, 1] * s[:, 1] + H[0, 2]) / w, (H[1, 0] * s[:, 0] + H[1, 1] * s[:, 1] + H[1, 2]) / w], 1).astype(np.float32)
    bad = np.zeros(n, bool)
    k = int(round(outliers * n))
    if k:
        bad[r.choice(n, k, replace=False)] = True
        dst[bad] = r.uniform(0, 2048, (k, 2)).astype(np.float32)
    return src, dst, ~bad, H


def apply(H, pts):
    """float64 (n, 2): the model applied to float32 points, for the truth tests"""
    H = np.asarray(H, np.float64).reshape(3, 3)
    p = np.asarray(pts, np.float64).reshape(-1, 2)
    w = H[2, 0] * p[:, 0] + H[2, 1] * p[:, 1] + H[2, 2]
    return np.stack([(H[0, 0] * p[:, 0] + H[0, 1] * p[:, 1] + H[0, 2]) / w, (H[1, 0] * p[:, 0] + H[1, 1] * p[:, 1] + H[1, 2]) / w], 1)
