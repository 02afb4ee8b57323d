"""The statement of robust rigid 3-D motion between paired 3-D points as this library defines it, in Python
and numpy: the oracle of tests/test_rigid_abi.py, tests/test_gpu_rigid.py and tests/test_gpu_rigid_py.py.  The product never imports
this file, and this file imports nothing of the product (the sampler and the stop table are those of tests/model_restate.py).  The
library must equal it bit for bit in the best hypothesis, its index, the three counts and the inlier bytes; the refit is compared
within the tolerance of tests/rigid_cases.py, because the device adds its sums in a free order.

Every floating-point value is an IEEE double; every expression is written with explicit parentheses in the one order that counts.

  pairs       src, dst float32 (n, 3); pair i is usable when both points are: three finite floats, not all three zero.  The pair list
              is the usable pairs in index order, each with its original index; n_usable is its length.
  tracks      two XYZ images float32 (h, w, 3), prev_pts float32 (n, 2), rows uint32 (n, 4) = x, y, err (float32 bits), status.
              Track i gives the pair (image 0 at prev_pts[i], image 1 at its row's x, y) when its status is not 0, its four
              coordinates are finite, both positions round to a pixel inside the image - ix = floor(x + 0.5) in float32, admitted
              iff x >= -0.5 and x < w - 0.5 - and both points are usable.
  sampling    sample(n_usable, 3, seed, j) of tests/model_restate.py.
  hypothesis  on each side e1 = p1 - p0, e2 = p2 - p0, c = e1 x e2 (each component (a b) - (c d)), l2 = (c0 c0 + c1 c1) + c2 c2,
              a = e1.e1 and b = e2.e2 summed the same way; void unless l2 > 1e-12 (a b) on both sides; u1 = e1 / sqrt(a),
              u3 = c / sqrt(l2), u2 = u3 x u1; v1 v2 v3 likewise on the destination side.  R[r][c] = (v1[r] u1[c] + v2[r] u2[c])
              + v3[r] u3[c]; cp = ((p0 + p1) + p2) / 3, cq likewise; t[r] = cq[r] - ((R[r][0] cp[0] + R[r][1] cp[1]) + R[r][2] cp[2]);
              void when one of the twelve numbers is not finite.
  scoring     m[r] = ((R[r][0] x + R[r][1] y) + R[r][2] z) + t[r].  EUCLID: inlier iff (dx dx + dy dy) + dz dz <= T T, d = m - q.
              DISPARITY (f = focal_px, fb = f baseline): an outlier unless m_z > 0 and q_z > 0; du = f ((m_x / m_z) - (q_x / q_z)),
              dv likewise with y, dd = fb ((1 / m_z) - (1 / q_z)); inlier iff (du du + dv dv) + dd dd <= T T.  The best hypothesis has
              the largest count, the lowest j among equals.  No valid hypothesis, or a best count below 3: no model.
  rounds      as section 4.30 with a sample size of 3; with fewer than 3 usable pairs nothing is searched.
  refit       over the inlier set, u = p - p0, v = q - q0 (the best sample's first pair): the count k and seventeen sums - u (3),
              v (3), u v^T (9), |u|^2, |v|^2; the centred cross-covariance C = Suv - (Su Sv^T) / k; Horn's symmetric 4 x 4; its
              largest eigenvector by cyclic Jacobi (JACOBI_SWEEPS sweeps) is the rotation's quaternion; t = q_mean - R p_mean; the
              rms residual from the same sums.  Degenerate - the two largest eigenvalues closer than 1e-12 of the largest - or not
              finite: the best hypothesis stands."""
import math

import numpy as np

from model_restate import AFFINE, ROUND, sample, stop_table

EUCLID, DISPARITY = 0, 1
VOID_SIN2 = 1e-12
REFIT_EPS = 1e-12
JACOBI_SWEEPS = 12


def usable(pts):
    """bool (n,): three finite floats that are not all zero"""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.isfinite(pts).all(1) & ~((pts == 0).all(1))


def pairs_of(src, dst):
    """(src float32 (k, 3), dst float32 (k, 3), original indices int32 (k,)): the usable pairs in index order"""
    src, dst = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(dst, np.float32).reshape(-1, 3)
    idx = np.flatnonzero(usable(src) & usable(dst)).astype(np.int32)
    return np.ascontiguousarray(src[idx]), np.ascontiguousarray(dst[idx]), idx


def pixel(x, extent):
    """the nearest pixel of a float32 coordinate, or None when it lies outside"""
    x = np.float32(x)
    if not (x >= np.float32(-0.5) and x < np.float32(extent) - np.float32(0.5)):
        return None
    return int(np.floor(x + np.float32(0.5)))


def track_pairs(xyz0, xyz1, prev_pts, rows):
    """(src (n, 3), dst (n, 3)) float32 of the n tracks, three zeros on both sides where a track gives no pair - so that pairs_of keeps
    the track's index"""
    xyz0, xyz1 = np.asarray(xyz0, np.float32), np.asarray(xyz1, np.float32)
    h, w = xyz0.shape[:2]
    prev_pts, rows = np.asarray(prev_pts, np.float32).reshape(-1, 2), np.asarray(rows, np.uint32).reshape(-1, 4)
    n = len(rows)
    src, dst = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    cur = rows[:, :2].copy().view(np.float32)
    for i in range(n):
        if rows[i, 3] == 0:
            continue
        c = [prev_pts[i, 0], prev_pts[i, 1], cur[i, 0], cur[i, 1]]
        if not all(np.isfinite(v) for v in c):
            continue
        px = [pixel(c[0], w), pixel(c[1], h), pixel(c[2], w), pixel(c[3], h)]
        if any(v is None for v in px):
            continue
        p, q = xyz0[px[1], px[0]], xyz1[px[3], px[2]]
        if usable(p)[0] and usable(q)[0]:
            src[i], dst[i] = p, q
    return src, dst


# ---- hypothesis ------------------------------------------------------------------------------------------------------------------------
def frame(p0, p1, p2):
    """rows u1 u2 u3 of the triad's orthonormal frame, or None when it is collinear; the points are triples of Python floats"""
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
    la, lc = math.sqrt(a), math.sqrt(l2)
    u1 = [e1[0] / la, e1[1] / la, e1[2] / la]
    u3 = [c0 / lc, c1 / lc, c2 / lc]
    u2 = [(u3[1] * u1[2]) - (u3[2] * u1[1]), (u3[2] * u1[0]) - (u3[0] * u1[2]), (u3[0] * u1[1]) - (u3[1] * u1[0])]
    return [u1, u2, u3]


def motion_from(p, q):
    """twelve floats (R row-major, t) or None; p, q: three triples of Python floats each"""
    U = frame(p[0], p[1], p[2])
    if U is None:
        return None
    V = frame(q[0], q[1], q[2])
    if V is None:
        return None
    R = [((V[0][r] * U[0][c]) + (V[1][r] * U[1][c])) + (V[2][r] * U[2][c]) for r in range(3) for c in range(3)]
    cp = [((p[0][c] + p[1][c]) + p[2][c]) / 3.0 for c in range(3)]
    cq = [((q[0][c] + q[1][c]) + q[2][c]) / 3.0 for c in range(3)]
    t = [cq[r] - (((R[r * 3] * cp[0]) + (R[r * 3 + 1] * cp[1])) + (R[r * 3 + 2] * cp[2])) for r in range(3)]
    M = R + t
    if not all(math.isfinite(v) for v in M):
        return None
    return M


def hypothesis(src, dst, seed, j):
    """(sample of three indices, -1 where none; twelve floats or None when void) over usable pairs"""
    s, complete = sample(len(src), 3, seed, j)
    if not complete:
        return s[:3], None
    p = [[float(v) for v in src[i]] for i in s[:3]]
    q = [[float(v) for v in dst[i]] for i in s[:3]]
    with np.errstate(all="ignore"):
        return s[:3], motion_from(p, q)


def inliers(M, metric, src, dst, t, camera=None):
    """bool (n,): the same expression on every pair, float64"""
    x, y, z = (np.asarray(src[:, k], np.float64) for k in range(3))
    qx, qy, qz = (np.asarray(dst[:, k], np.float64) for k in range(3))
    M = [np.float64(v) for v in M]
    t2 = np.float64(t) * np.float64(t)
    with np.errstate(all="ignore"):
        mx = (((M[0] * x) + (M[1] * y)) + (M[2] * z)) + M[9]
        my = (((M[3] * x) + (M[4] * y)) + (M[5] * z)) + M[10]
        mz = (((M[6] * x) + (M[7] * y)) + (M[8] * z)) + M[11]
        if metric == DISPARITY:
            f = np.float64(camera[0])
            fb = f * np.float64(camera[1])
            du = f * ((mx / mz) - (qx / qz))
            dv = f * ((my / mz) - (qy / qz))
            dd = fb * ((1.0 / mz) - (1.0 / qz))
            return (mz > 0) & (qz > 0) & (((du * du) + (dv * dv)) + (dd * dd) <= t2)
        dx, dy, dz = mx - qx, my - qy, mz - qz
        return ((dx * dx) + (dy * dy)) + (dz * dz) <= t2


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


def refit_sums(src, dst, keep, p0, q0, order="index"):
    """(k, the seventeen sums) over the kept pairs"""
    keep = np.asarray(keep).reshape(-1) != 0
    p = np.asarray(src, np.float32)[keep].astype(np.float64)
    q = np.asarray(dst, np.float32)[keep].astype(np.float64)
    u = [p[:, c] - float(p0[c]) for c in range(3)]
    v = [q[:, c] - float(q0[c]) for c in range(3)]
    cols = u + v + [u[r] * v[c] for r in range(3) for c in range(3)]
    cols.append(((u[0] * u[0]) + (u[1] * u[1])) + (u[2] * u[2]))
    cols.append(((v[0] * v[0]) + (v[1] * v[1])) + (v[2] * v[2]))
    return len(p), [_sum(a, order) for a in cols]


def jacobi4(N):
    """eigenvalues and eigenvectors (columns of V) of a symmetric 4 x 4 by cyclic Jacobi"""
    A = [list(r) for r in N]
    V = [[1.0 if r == c else 0.0 for c in range(4)] for r in range(4)]
    for _ in range(JACOBI_SWEEPS):
        for p in range(3):
            for q in range(p + 1, 4):
                apq = A[p][q]
                if apq == 0.0 or not math.isfinite(apq):
                    continue
                theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                t = 1.0 / (abs(theta) + math.sqrt((theta * theta) + 1.0))
                if theta < 0:
                    t = -t
                c = 1.0 / math.sqrt((t * t) + 1.0)
                s = t * c
                app, aqq = A[p][p], A[q][q]
                A[p][p] = app - (t * apq)
                A[q][q] = aqq + (t * apq)
                A[p][q] = A[q][p] = 0.0
                for r in range(4):
                    if r in (p, q):
                        continue
                    arp, arq = A[r][p], A[r][q]
                    A[r][p] = A[p][r] = (c * arp) - (s * arq)
                    A[r][q] = A[q][r] = (s * arp) + (c * arq)
                for k in range(4):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = (c * vkp) - (s * vkq)
                    V[k][q] = (s * vkp) + (c * vkq)
    return [A[i][i] for i in range(4)], V


def rms_of(k, S, p0, q0, M):
    """the rms residual of the motion M over the summed pairs: r_i = (R u_i - v_i) + e0, e0 = (R p0 + t) - q0"""
    kk = float(k)
    e0 = [((((M[r * 3] * p0[0]) + (M[r * 3 + 1] * p0[1])) + (M[r * 3 + 2] * p0[2])) + M[9 + r]) - q0[r] for r in range(3)]
    Rsu = [((M[r * 3] * S[0]) + (M[r * 3 + 1] * S[1])) + (M[r * 3 + 2] * S[2]) for r in range(3)]
    cross = 0.0
    for r in range(3):
        for c in range(3):
            cross = cross + (M[r * 3 + c] * S[6 + c * 3 + r])
    ss = (S[15] + S[16]) - (2.0 * cross)
    ss = ss + (2.0 * ((((e0[0] * Rsu[0]) + (e0[1] * Rsu[1])) + (e0[2] * Rsu[2])) - (((e0[0] * S[3]) + (e0[1] * S[4])) + (e0[2] * S[5]))))
    ss = ss + (kk * (((e0[0] * e0[0]) + (e0[1] * e0[1])) + (e0[2] * e0[2])))
    rms = math.sqrt((ss if ss > 0 else 0.0) / kk)
    return rms if math.isfinite(rms) else 0.0


def refit_close(k, S, p0, q0, best):
    """31 floats: refit R t, `best` R t, the two centroids, rms.  best None (the refit alone): a degenerate refit gives None."""
    if k < 3:
        return None
    p0, q0 = [float(v) for v in p0], [float(v) for v in q0]
    with np.errstate(all="ignore"):
        kk = float(k)
        cp = [p0[c] + (S[c] / kk) for c in range(3)]
        cq = [q0[c] + (S[3 + c] / kk) for c in range(3)]
        C = [[S[6 + r * 3 + c] - ((S[r] * S[3 + c]) / kk) for c in range(3)] for r in range(3)]
        N = [[0.0] * 4 for _ in range(4)]
        N[0][0] = (C[0][0] + C[1][1]) + C[2][2]
        N[1][1] = (C[0][0] - C[1][1]) - C[2][2]
        N[2][2] = (C[1][1] - C[0][0]) - C[2][2]
        N[3][3] = (C[2][2] - C[0][0]) - C[1][1]
        N[0][1] = N[1][0] = C[1][2] - C[2][1]
        N[0][2] = N[2][0] = C[2][0] - C[0][2]
        N[0][3] = N[3][0] = C[0][1] - C[1][0]
        N[1][2] = N[2][1] = C[0][1] + C[1][0]
        N[1][3] = N[3][1] = C[2][0] + C[0][2]
        N[2][3] = N[3][2] = C[1][2] + C[2][1]
        lam, V = jacobi4(N)
        hi = 0
        for i in (1, 2, 3):
            if lam[i] > lam[hi]:
                hi = i
        second = 1 if hi == 0 else 0
        for i in range(4):
            if i != hi and lam[i] > lam[second]:
                second = i
        M = None
        if lam[hi] - lam[second] > REFIT_EPS * abs(lam[hi]):
            w, x, y, z = V[0][hi], V[1][hi], V[2][hi], V[3][hi]
            ln = math.sqrt((((w * w) + (x * x)) + (y * y)) + (z * z))
            w, x, y, z = w / ln, x / ln, y / ln, z / ln
            M = [(((w * w) + (x * x)) - (y * y)) - (z * z), 2.0 * ((x * y) - (w * z)), 2.0 * ((x * z) + (w * y)),
                 2.0 * ((x * y) + (w * z)), (((w * w) - (x * x)) + (y * y)) - (z * z), 2.0 * ((y * z) - (w * x)),
                 2.0 * ((x * z) - (w * y)), 2.0 * ((y * z) + (w * x)), (((w * w) - (x * x)) - (y * y)) + (z * z)]
            M += [cq[r] - (((M[r * 3] * cp[0]) + (M[r * 3 + 1] * cp[1])) + (M[r * 3 + 2] * cp[2])) for r in range(3)]
            if not all(math.isfinite(v) for v in M):
                M = None
        if M is None:
            if best is None:
                return None
            M = list(best)
        return M + ([0.0] * 12 if best is None else list(best)) + cp + cq + [rms_of(k, S, p0, q0, M)]


def refit(src, dst, keep=None, order="index"):
    """the refit alone, about the first kept pair: 31 floats (the hypothesis slots zero) or None"""
    src, dst = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(dst, np.float32).reshape(-1, 3)
    keep = np.ones(len(src), bool) if keep is None else np.asarray(keep).reshape(-1) != 0
    if not keep.any():
        return None
    first = np.flatnonzero(keep)[0]
    k, S = refit_sums(src, dst, keep, src[first], dst[first], order)
    return refit_close(k, S, src[first], dst[first], None)


# ---- the whole search -------------------------------------------------------------------------------------------------------------------
def fit(src, dst, metric=EUCLID, threshold=0.02, camera=None, max_iters=1000, confidence=0.99, seed=0, order="index"):
    """dict: found, result (31 floats; zeros when no model), best_j (-1 when none), n_usable, n_inliers, n_hypotheses, inliers (uint8
    (n,) of 0 / 1 by original index), void (hypotheses taken that were void)"""
    n_given = len(np.asarray(src).reshape(-1, 3))
    P, Q, idx = pairs_of(src, dst)
    n = len(P)
    out = {"found": False, "result": [0.0] * 31, "best_j": -1, "n_usable": n, "n_inliers": 0, "n_hypotheses": 0, "inliers": np.zeros(n_given, np.uint8), "void": 0}
    if n < 3:
        return out
    need = stop_table(n, AFFINE, confidence, max_iters)
    best, best_j, B, taken, void = -1, -1, None, 0, 0
    for r in range(len(need)):
        end = min((r + 1) * ROUND, max_iters)
        for j in range(r * ROUND, end):
            _, M = hypothesis(P, Q, seed, j)
            if M is None:
                void += 1
                continue
            c = int(inliers(M, metric, P, Q, threshold, camera).sum())
            if c > best:
                best, best_j, B = c, j, M
        taken = end
        if best >= need[r]:
            break
    out["n_hypotheses"], out["void"] = taken, void
    if best < 3:
        return out
    keep = inliers(B, metric, P, Q, threshold, camera)
    s, _ = sample(n, 3, seed, best_j)
    p0, q0 = P[s[0]], Q[s[0]]
    k, S = refit_sums(P, Q, keep, p0, q0, order)
    out.update(found=True, result=refit_close(k, S, p0, q0, B), best_j=best_j, n_inliers=int(keep.sum()))
    out["inliers"][idx[keep]] = 1
    return out


def fit_tracks(xyz0, xyz1, prev_pts, rows, **kw):
    src, dst = track_pairs(xyz0, xyz1, prev_pts, rows)
    return fit(src, dst, **kw)


def bits(v):
    return np.array(v, np.float64).view(np.uint64)
