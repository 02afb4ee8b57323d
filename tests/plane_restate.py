"""The statement of robust plane fitting to 3-D points as this library defines it, in Python and numpy: the
oracle of tests/test_plane_abi.py, tests/test_gpu_plane.py and tests/test_gpu_plane_py.py.  The product never imports this file,
and this file imports nothing of the product (the sampler, the mixer and the stop table are those of tests/model_restate.py).
The library must equal it bit for bit in the best hypothesis, its index, the three counts and the inlier image; the refit is
compared within the tolerance of tests/plane_cases.py, because the device adds its sums in a free order.

Every floating-point value is an IEEE double; every expression is written with explicit parentheses in the one order that counts.

  points      xyz float32 (h, w, 3); a pixel is a candidate inside the box (x0, y0, rw, rh; default the image) whose mask byte (if a
              mask is given) is not 0; a candidate is usable when its three floats are finite and not all three zero.  The point list
              is the usable candidates in raster order, each with its pixel index y w + x; n is its length.
  sampling    sample(n, 3, seed, j) of tests/model_restate.py.
  hypothesis  e1 = p1 - p0, e2 = p2 - p0, c = e1 x e2 (each component (a b) - (c d)), l2 = (c0 c0 + c1 c1) + c2 c2, a = e1.e1 and
              b = e2.e2 summed the same way; void unless l2 > 1e-12 (a b); normal = c / sqrt(l2); d = -((n0 p0x + n1 p0y) + n2 p0z);
              d < 0: all four negated; void when d == 0 or a number is not finite; ALONG_Z: void unless |n2| > 1e-6.
  scoring     e = ((n0 x + n1 y) + n2 z) + d; PERP: inlier iff e e <= t t; ALONG_Z: inlier iff e e <= (t t) (n2 n2).  The best hypothesis
              has the largest count, the lowest j among equals.  No valid hypothesis, or a best count below 3: no model.
  rounds      as section 4.30 with a sample size of 3; with fewer than 3 points nothing is searched and no hypothesis is taken.
  refit       over the inlier set, u = p - p0 (the best sample's first point): the count k, the three sums and the six sums of
              products; the centred scatter C = S2 - (S1 S1) / k.  PERP: the eigenvector of C's smallest eigenvalue by cyclic Jacobi
              (JACOBI_SWEEPS sweeps); ALONG_Z: the regression of z on x and y by Cramer's rule.  Oriented towards the camera; a
              degenerate refit falls back to the best hypothesis."""
import math

import numpy as np

from model_restate import AFFINE, ROUND, sample, stop_table

PERP, ALONG_Z = 0, 1
VOID_SIN2 = 1e-12            # l2 > VOID_SIN2 (a b): the sine of the sample's angle above 1e-6
MIN_NZ = 1e-6
REFIT_EPS = 1e-12
JACOBI_SWEEPS = 8


def points_of(xyz, box=None, mask=None):
    """(float32 (n, 3), int32 pixel indices (n,)): the usable candidates in raster order"""
    xyz = np.asarray(xyz)
    h, w = xyz.shape[:2]
    x0, y0, rw, rh = (0, 0, w, h) if box is None else box
    cand = np.zeros((h, w), bool)
    cand[y0:y0 + rh, x0:x0 + rw] = True
    if mask is not None:
        cand &= np.asarray(mask)[:h, :w] != 0
    with np.errstate(all="ignore"):
        usable = cand & np.isfinite(xyz).all(2) & ~((xyz == 0).all(2))
    idx = np.flatnonzero(usable.reshape(-1)).astype(np.int32)
    return np.ascontiguousarray(xyz.reshape(-1, 3)[idx], np.float32), idx


def plane_from(p0, p1, p2, metric):
    """four floats or None; the points are triples of Python floats"""
    e1 = [p1[k] - p0[k] for k in range(3)]
    e2 = [p2[k] - p0[k] for k in range(3)]
    c0 = (e1[1] * e2[2]) - (e1[2] * e2[1])
    c1 = (e1[2] * e2[0]) - (e1[0] * e2[2])
    c2 = (e1[0] * e2[1]) - (e1[1] * e2[0])
    l2 = ((c0 * c0) + (c1 * c1)) + (c2 * c2)
    a = ((e1[0] * e1[0]) + (e1[1] * e1[1])) + (e1[2] * e1[2])
    b = ((e2[0] * e2[0]) + (e2[1] * e2[1])) + (e2[2] * e2[2])
    if not l2 > VOID_SIN2 * (a * b):
        return None
    ln = math.sqrt(l2)
    n0, n1, n2 = c0 / ln, c1 / ln, c2 / ln
    d = -(((n0 * p0[0]) + (n1 * p0[1])) + (n2 * p0[2]))
    if d < 0:
        n0, n1, n2, d = -n0, -n1, -n2, -d
    if d == 0 or not all(math.isfinite(v) for v in (n0, n1, n2, d)):
        return None
    if metric == ALONG_Z and not abs(n2) > MIN_NZ:
        return None
    return [n0, n1, n2, d]


def hypothesis(pts, metric, seed, j):
    """(sample of three indices, -1 where none; four floats or None when void)"""
    s, complete = sample(len(pts), 3, seed, j)
    if not complete:
        return s[:3], None
    p = [[float(v) for v in pts[i]] for i in s[:3]]
    with np.errstate(all="ignore"):
        return s[:3], plane_from(p[0], p[1], p[2], metric)


def inliers(P, metric, pts, t):
    """bool (n,): the same expression on every point, float64"""
    x, y, z = (np.asarray(pts[:, k], np.float64) for k in range(3))
    n0, n1, n2, d = (np.float64(v) for v in P)
    t2 = np.float64(t) * np.float64(t)
    with np.errstate(all="ignore"):
        e = (((n0 * x) + (n1 * y)) + (n2 * z)) + d
        lim = t2 * (n2 * n2) if metric == ALONG_Z else t2
        return e * e <= lim


# ---- refit -----------------------------------------------------------------------------------------------------------------------------
def _sum(v, order):
    v = np.asarray(v, np.float64)
    if order == "reversed":
        v = v[::-1]
    if order == "pairwise":
        v = list(v)
        while len(v) > 1:
            v = [v[i] + v[i + 1] if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
        return float(v[0]) if v else 0.0
    return float(np.add.accumulate(np.concatenate([[0.0], v]))[-1])


def refit_sums(pts, keep, p0, order="index"):
    """(k, [Su, Sv, Sw, Suu, Suv, Suw, Svv, Svw, Sww]) over the kept points, u = p - p0"""
    q = np.asarray(pts, np.float32)[np.asarray(keep).reshape(-1) != 0].astype(np.float64)
    u, v, w = q[:, 0] - float(p0[0]), q[:, 1] - float(p0[1]), q[:, 2] - float(p0[2])
    return len(q), [_sum(a, order) for a in (u, v, w, u * u, u * v, u * w, v * v, v * w, w * w)]


def jacobi3(C):
    """eigenvalues and eigenvectors (columns of V) of a symmetric 3 x 3 by cyclic Jacobi, JACOBI_SWEEPS sweeps over (0,1) (0,2) (1,2)"""
    A = [list(r) for r in C]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(JACOBI_SWEEPS):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = A[p][q]
            if apq == 0.0 or not math.isfinite(apq):
                continue
            theta = (A[q][q] - A[p][p]) / (2.0 * apq)
            t = 1.0 / (abs(theta) + math.sqrt((theta * theta) + 1.0))
            if theta < 0:
                t = -t
            c = 1.0 / math.sqrt((t * t) + 1.0)
            s = t * c
            r = 3 - p - q
            app, aqq, arp, arq = A[p][p], A[q][q], A[r][p], A[r][q]
            A[p][p] = app - (t * apq)
            A[q][q] = aqq + (t * apq)
            A[p][q] = A[q][p] = 0.0
            A[r][p] = A[p][r] = (c * arp) - (s * arq)
            A[r][q] = A[q][r] = (s * arp) + (c * arq)
            for k in range(3):
                vkp, vkq = V[k][p], V[k][q]
                V[k][p] = (c * vkp) - (s * vkq)
                V[k][q] = (s * vkp) + (c * vkq)
    return [A[0][0], A[1][1], A[2][2]], V


def refit_close(k, S, p0, metric, best):
    """twelve floats: plane 4, `best` 4, centroid 3, rms.  best None (the refit alone): a degenerate refit gives None."""
    out_best = [0.0] * 4 if best is None else list(best)
    if k < 3:
        return None
    with np.errstate(all="ignore"):
        kk = float(k)
        mu = [S[0] / kk, S[1] / kk, S[2] / kk]
        cen = [float(p0[0]) + mu[0], float(p0[1]) + mu[1], float(p0[2]) + mu[2]]
        Cuu, Cuv, Cuw = S[3] - ((S[0] * S[0]) / kk), S[4] - ((S[0] * S[1]) / kk), S[5] - ((S[0] * S[2]) / kk)
        Cvv, Cvw, Cww = S[6] - ((S[1] * S[1]) / kk), S[7] - ((S[1] * S[2]) / kk), S[8] - ((S[2] * S[2]) / kk)
        plane, rms = None, 0.0
        if metric == PERP:
            lam, V = jacobi3([[Cuu, Cuv, Cuw], [Cuv, Cvv, Cvw], [Cuw, Cvw, Cww]])
            lo = 0
            for i in (1, 2):
                if lam[i] < lam[lo]:
                    lo = i
            hi = 0
            for i in (1, 2):
                if lam[i] > lam[hi]:
                    hi = i
            mid = 3 - lo - hi if lo != hi else -1
            if mid >= 0 and lam[mid] > REFIT_EPS * lam[hi]:            # else the inliers lie on a line (or are one point)
                n = [V[0][lo], V[1][lo], V[2][lo]]
                ln = math.sqrt(((n[0] * n[0]) + (n[1] * n[1])) + (n[2] * n[2]))
                n = [n[0] / ln, n[1] / ln, n[2] / ln]
                d = -(((n[0] * cen[0]) + (n[1] * cen[1])) + (n[2] * cen[2]))
                plane = [n[0], n[1], n[2], d]
                rms = math.sqrt((lam[lo] if lam[lo] > 0 else 0.0) / kk)
        else:
            det = (Cuu * Cvv) - (Cuv * Cuv)
            if det > REFIT_EPS * (Cuu * Cvv):
                a = ((Cuw * Cvv) - (Cvw * Cuv)) / det
                b = ((Cvw * Cuu) - (Cuw * Cuv)) / det
                ln = math.sqrt(((a * a) + (b * b)) + 1.0)
                d = (cen[2] - ((a * cen[0]) + (b * cen[1]))) / ln
                plane = [a / ln, b / ln, -1.0 / ln, d]
                ss = ((Cww - (2.0 * ((a * Cuw) + (b * Cvw)))) + (((a * a) * Cuu) + ((b * b) * Cvv))) + ((2.0 * (a * b)) * Cuv)
                rms = math.sqrt((ss if ss > 0 else 0.0) / kk)
        if plane is not None and plane[3] < 0:
            plane = [-v for v in plane]
        if plane is None or not all(math.isfinite(v) for v in plane + [rms]) or not plane[3] > 0:
            if best is None:
                return None
            # the best hypothesis stands; its residual from the same sums: e_i = n.u_i + e0 (ALONG_Z: divided by |n2|)
            n, e0 = best[:3], (((best[0] * float(p0[0])) + (best[1] * float(p0[1]))) + (best[2] * float(p0[2]))) + best[3]
            q = ((((n[0] * n[0]) * S[3]) + ((n[1] * n[1]) * S[6])) + ((n[2] * n[2]) * S[8])) + \
                (2.0 * ((((n[0] * n[1]) * S[4]) + ((n[0] * n[2]) * S[5])) + ((n[1] * n[2]) * S[7])))
            ss = (q + ((2.0 * e0) * (((n[0] * S[0]) + (n[1] * S[1])) + (n[2] * S[2])))) + ((kk * e0) * e0)
            if metric == ALONG_Z:
                ss = ss / (n[2] * n[2])
            rms = math.sqrt((ss if ss > 0 else 0.0) / kk)
            if not math.isfinite(rms):
                rms = 0.0
            plane = list(best)
    return plane + out_best + cen + [rms]


def refit(pts, keep, metric, order="index"):
    """the refit alone, about the first kept point: twelve floats (the hypothesis slots zero) or None"""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    keep = np.ones(len(pts), bool) if keep is None else np.asarray(keep).reshape(-1) != 0
    if not keep.any():
        return None
    p0 = pts[np.flatnonzero(keep)[0]]
    k, S = refit_sums(pts, keep, p0, order)
    return refit_close(k, S, p0, metric, None)


# ---- the whole search -------------------------------------------------------------------------------------------------------------------
def fit(xyz, box=None, mask=None, metric=PERP, threshold=0.02, max_iters=1000, confidence=0.99, seed=0, order="index"):
    """dict: found, result (12 floats: refit plane, best hypothesis, centroid, rms; zeros when no model), best_j (-1 when none),
    n_usable, n_inliers, n_hypotheses, inliers (uint8 h x w of 0 / 255), void (hypotheses taken that were void)"""
    xyz = np.asarray(xyz, np.float32)
    h, w = xyz.shape[:2]
    pts, idx = points_of(xyz, box, mask)
    n = len(pts)
    out = {"found": False, "result": [0.0] * 12, "best_j": -1, "n_usable": n, "n_inliers": 0, "n_hypotheses": 0,
           "inliers": np.zeros((h, w), np.uint8), "void": 0}
    if n < 3:
        return out
    need = stop_table(n, AFFINE, confidence, max_iters)
    best, best_j, B, taken, void = -1, -1, None, 0, 0
    for r in range(len(need)):
        end = min((r + 1) * ROUND, max_iters)
        for j in range(r * ROUND, end):
            _, P = hypothesis(pts, metric, seed, j)
            if P is None:
                void += 1
                continue
            c = int(inliers(P, metric, pts, threshold).sum())
            if c > best:
                best, best_j, B = c, j, P
        taken = end
        if best >= need[r]:
            break
    out["n_hypotheses"], out["void"] = taken, void
    if best < 3:
        return out
    keep = inliers(B, metric, pts, threshold)
    s, _ = sample(n, 3, seed, best_j)
    p0 = pts[s[0]]
    k, S = refit_sums(pts, keep, p0, order)
    out.update(found=True, result=refit_close(k, S, p0, metric, B), best_j=best_j, n_inliers=int(keep.sum()))
    out["inliers"].reshape(-1)[idx[keep]] = 255
    return out


def bits(v):
    return np.array(v, np.float64).view(np.uint64)
