"""The cases shared by the rigid-motion suites (tests/test_rigid_statement.py, test_rigid_abi.py, test_gpu_rigid.py,
test_gpu_rigid_py.py): small sets of paired 3-D points from seeded generators, and track sets into two small XYZ images, each with
its metric, threshold, camera, seed, max_iters and confidence; the statement's answer per case, computed once; one caller for the
entries of libvp; and the bounds and tolerances, which are measured on the statement alone."""
import ctypes as C
import functools
import math

import numpy as np

import rigid_restate as R

EUCLID, DISPARITY = R.EUCLID, R.DISPARITY

# ---- the refit tolerance -------------------------------------------------------------------------------------------------------------------
# The device adds the count and the seventeen refit sums in a free order, so the refit is compared within a tolerance.  It is measured
# on the statement: for every case the restatement's refit runs with its sums in index order, reversed and pairwise; SPREAD is the
# largest difference, over the cases, of the angle between the rotations, |t' - t| / max(1, |t|), the larger of the two centroid
# differences and |rms' - rms|; the tolerance is 64 times the spread (the device groups by waves and blocks, not by pairs), with a
# floor of 16 ulp of the compared quantity.  tests/test_rigid_statement.py measures the spreads again and compares them with these.
SPREAD_ROT = 1.2100532712857476e-15
SPREAD_T = 2.4993891989072927e-15
SPREAD_CENTROID = 0.0            # the floor applies: 16 ulp of the centroid's length
SPREAD_RMS = 1.723138992604234e-12
TOL_ROT, TOL_T, TOL_CENTROID, TOL_RMS = 64 * SPREAD_ROT, 64 * SPREAD_T, 64 * SPREAD_CENTROID, 64 * SPREAD_RMS

# ---- how well the generating motion comes back ---------------------------------------------------------------------------------------------
# Measured on the statement with threshold = 4 sigma at the four sigmas below (the cases noise_sigma_*; 400 pairs, 30 % outliers) and on
# every other case that has a generating motion: the largest error divided by the case's sigma - the rotation angle (radians per
# unit of sigma) and |t - t_true| (units per unit of sigma) of the refit and of the best three-pair hypothesis.  A case passes under
# twice the measured ratio times its sigma: one seed is one draw.  tests/test_rigid_statement.py prints the figures per case.
SIGMAS = (0.001, 0.003, 0.01, 0.03)
RECOVER_REFIT_ROT = 0.4113875014568486           # measured: the largest over the cases (usable_65)
RECOVER_REFIT_T = 1.054700933588865              # outliers_90_cut_at_44
RECOVER_HYP_ROT = 2.0139201620655753             # usable_64
RECOVER_HYP_T = 2.624029021224069                # outliers_90_cut_at_44; the four sigma cases alone: 0.168, 0.325, 0.908, 2.465
# A mirrored destination set holds no rotation: the most pairs any hypothesis of the case `mirrored` gathers, measured on the
# statement, and the cap the suites assert - twice that, far below the half of the pairs a wrong answer would need
MIRROR_MEASURED = 10                             # of 300 pairs, among 512 hypotheses
MIRROR_CAP = 2 * MIRROR_MEASURED


def library():
    from vision import _vp
    lib = C.CDLL(_vp.LIB_PATH)
    for name, (res, args) in _vp._SIGS.items():
        if name.startswith(("vp_fit_rigid_", "vp_rigid_")) or name == "vp_last_error":
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


@functools.lru_cache(maxsize=None)
def geometry(n=4096):
    """(workspace bytes, geometry[8]) of vp_fit_rigid_plan"""
    ws, g = C.c_size_t(0), np.zeros(8, np.int32)
    assert library().vp_fit_rigid_plan(n, C.addressof(ws), g.ctypes.data) == 0
    return ws.value, g


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------
def rotation(rx, ry, rz):
    """Rodrigues' rotation of the vector (rx, ry, rz), float64"""
    v = np.array([rx, ry, rz], np.float64)
    a = float(np.linalg.norm(v))
    if a == 0:
        return np.eye(3)
    k = v / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)


MOTION_1 = (rotation(0.05, -0.12, 0.08), np.array([0.30, -0.10, 0.20]))
MOTION_2 = (rotation(-0.2, 0.1, 0.3), np.array([-0.25, 0.30, -0.10]))


def pairs(n, motions, shares, sigma, outliers, seed, threshold=None):
    """(src, dst float32 (n, 3), label (n,)): sources uniform in [-1, 1]^2 x [1, 3]; the share shares[i] of the pairs moves by
    motions[i] = (R, t) with noise uniform in [-2 sigma, 2 sigma] per axis (inside a threshold of 4 sigma: 2 sqrt(3) < 4); the share
    `outliers` lands 10 to 30 thresholds away from where motions[0] would put it; label: the motion's number, -1 for an outlier"""
    r = np.random.default_rng(5200 + seed)
    T = 4 * sigma if threshold is None else threshold
    src = np.stack([r.uniform(-1, 1, n), r.uniform(-1, 1, n), r.uniform(1, 3, n)], 1)
    label = np.full(n, -1)
    order = r.permutation(n)
    rest = order[int(round(outliers * n)):]
    cuts = np.round(np.cumsum(shares) / np.sum(shares) * len(rest)).astype(int)
    lo = 0
    for i, hi in enumerate(cuts):
        label[rest[lo:hi]] = i
        lo = hi
    d = r.normal(size=(n, 3))
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * r.uniform(10 * T, 30 * T, (n, 1))
    dst = src @ motions[0][0].T + motions[0][1] + d
    for i, (Rm, t) in enumerate(motions):
        m = label == i
        dst[m] = src[m] @ Rm.T + t + r.uniform(-2 * sigma, 2 * sigma, (int(m.sum()), 3))
    return src.astype(np.float32), dst.astype(np.float32), label


class Case:
    def __init__(self, cid, src, dst, metric=EUCLID, threshold=0.012, camera=None, seed=0, max_iters=512, confidence=0.99, truth=None, good=None, gross=None,
                 sigma=None, found=True, tracks=None):
        self.id, self.metric, self.threshold, self.camera = cid, metric, threshold, camera
        self.src, self.dst = np.ascontiguousarray(src, np.float32).reshape(-1, 3), np.ascontiguousarray(dst, np.float32).reshape(-1, 3)
        self.seed, self.max_iters, self.confidence = seed, max_iters, confidence
        self.truth, self.good, self.gross, self.sigma, self.found = truth, good, gross, sigma, found     # the generating motion, its pairs, the gross outliers
        self.tracks = tracks              # None, or dict(xyz0, xyz1, prev, rows, pad0, pad1): src / dst are then what the statement samples
        self.src.flags.writeable = False
        self.dst.flags.writeable = False
        self.n = len(self.src)

    def kw(self):
        return dict(metric=self.metric, threshold=self.threshold, camera=self.camera, max_iters=self.max_iters, confidence=self.confidence, seed=self.seed)


SIGMA = 0.003
UNUSABLE = [(np.nan, 1.0, 2.0), (0.0, 0.0, 0.0), (1.0, np.inf, 2.0), (1.0, 2.0, -np.inf)]


def _with_unusable(src, dst, label, extra, seed):
    """`extra` unusable pairs - NaN, the three zeros, the infinities, on either side - inserted at random places, singly and in short
    runs, so that the usable pairs' runs are cut inside waves"""
    r = np.random.default_rng(77 + seed)
    n = len(src) + extra
    bad = np.zeros(n, bool)
    while bad.sum() < extra:
        at, ln = int(r.integers(0, n)), int(r.integers(1, 4))
        bad[at:at + min(ln, extra - int(bad.sum()))] = True
    bad[np.flatnonzero(bad)[extra:]] = False
    S, D, L = np.ones((n, 3), np.float32), np.ones((n, 3), np.float32), np.full(n, -2)
    S[~bad], D[~bad], L[~bad] = src, dst, label
    for k, i in enumerate(np.flatnonzero(bad)):
        (S if k % 2 else D)[i] = UNUSABLE[(k // 2) % 4]
    return S, D, L


def _truth_case(cid, n, outliers, scene_seed, sigma=SIGMA, motion=MOTION_1, extra=0, **kw):
    src, dst, label = pairs(n, [motion], [1], sigma, outliers, scene_seed)
    if extra:
        src, dst, label = _with_unusable(src, dst, label, extra, scene_seed)
    kw.setdefault("threshold", 4 * sigma)
    return Case(cid, src, dst, truth=motion, good=label == 0, gross=label == -1, sigma=sigma, **kw)


def _track_case(cid, w, h, n, pad0, pad1, scene_seed, **kw):
    """two XYZ images and n tracks: image 1 holds, at every track's end, the moved point of its start plus noise; then the special rows"""
    r = np.random.default_rng(6100 + scene_seed)
    xyz0 = np.stack([r.uniform(-1, 1, (h, w)), r.uniform(-1, 1, (h, w)), r.uniform(1, 3, (h, w))], 2).astype(np.float32)
    xyz1 = np.stack([r.uniform(-1, 1, (h, w)), r.uniform(-1, 1, (h, w)), r.uniform(1, 3, (h, w))], 2).astype(np.float32)
    Rm, t = MOTION_1
    prev = np.stack([r.uniform(-0.5, w - 0.51, n), r.uniform(-0.5, h - 0.51, n)], 1).astype(np.float32)
    cur = np.stack([r.uniform(-0.5, w - 0.51, n), r.uniform(-0.5, h - 0.51, n)], 1).astype(np.float32)
    special = {0: ("status", None), 1: ("nan", 0), 2: ("nan", 3), 3: ("x", -0.5), 4: ("x", -0.51), 5: ("x", w - 0.5), 6: ("x", 2.5), 7: ("y1", h - 0.5),
               8: ("zero0", None), 9: ("zero1", None), 10: ("y1", -0.5)}
    for i, (what, v) in special.items():
        if what == "x":
            prev[i, 0] = v
        elif what == "y1":
            cur[i, 1] = v
    for i in range(n):
        x0, y0, x1, y1 = (R.pixel(c, e) for c, e in ((prev[i, 0], w), (prev[i, 1], h), (cur[i, 0], w), (cur[i, 1], h)))
        if None in (x0, y0, x1, y1):
            continue
        xyz1[y1, x1] = (xyz0[y0, x0].astype(np.float64) @ Rm.T + t + r.uniform(-2 * SIGMA, 2 * SIGMA, 3)).astype(np.float32)
    rows = np.zeros((n, 4), np.uint32)
    rows[:, :2] = cur.view(np.uint32)
    rows[:, 2] = np.float32(0.25).view(np.uint32)
    rows[:, 3] = 1
    rows[0, 3] = 0
    prev[1, 0] = np.nan
    rows[2, 1] = np.float32(np.nan).view(np.uint32)
    p8 = (R.pixel(prev[8, 0], w), R.pixel(prev[8, 1], h))
    xyz0[p8[1], p8[0]] = 0
    c9 = (R.pixel(cur[9, 0], w), R.pixel(cur[9, 1], h))
    xyz1[c9[1], c9[0]] = 0
    rows[n // 2:n // 2 + 3, 3] = (0, 2, 0xFFFFFFFF)          # any status that is not 0 counts
    src, dst = R.track_pairs(xyz0, xyz1, prev, rows)
    kw.setdefault("threshold", 4 * SIGMA)
    return Case(cid, src, dst, tracks=dict(xyz0=xyz0, xyz1=xyz1, prev=prev, rows=rows, pad0=pad0, pad1=pad1, w=w, h=h), **kw)


CAMERA = (500.0, 0.1)


def _near_far(seed):
    """pairs at 1 m and at 8 m whose depth carries the quantisation of a disparity kept in sixteenths of a pixel, on both sides"""
    r = np.random.default_rng(seed)
    f, b = CAMERA
    n = 300
    Z = np.where(np.arange(n) % 2 == 0, 1.0, 8.0) + r.uniform(-0.1, 0.1, n)
    src = np.stack([r.uniform(-0.4, 0.4, n) * Z, r.uniform(-0.3, 0.3, n) * Z, Z], 1)
    dst = src @ MOTION_1[0].T + MOTION_1[1]

    def quantised(P):
        d = np.rint(f * b / P[:, 2] * 16) / 16
        z = f * b / d
        return np.stack([P[:, 0] / P[:, 2] * z, P[:, 1] / P[:, 2] * z, z], 1)
    return quantised(src).astype(np.float32), quantised(dst).astype(np.float32)


def _cases():
    out = []
    T = 4 * SIGMA
    g = geometry()[1]
    run, stage = int(g[0]), int(g[1])
    # the smallest inputs
    s3 = np.array([[0.5, 0.1, 2.0], [0, 0, 0], [-0.4, 0.3, 2.2], [0.1, -0.6, 1.9]], np.float32)
    d3 = (s3.astype(np.float64) @ MOTION_1[0].T + MOTION_1[1]).astype(np.float32)
    out.append(Case("three_pairs", s3, d3, max_iters=256))
    d2 = d3.copy(); d2[2] = 0
    out.append(Case("two_pairs", s3, d2, found=False))
    out.append(Case("none_zeros", np.zeros((5, 3), np.float32), np.ones((5, 3), np.float32), found=False))
    out.append(Case("none_nan", np.ones((5, 3), np.float32), np.full((5, 3), np.nan, np.float32), found=False))
    inf = np.ones((5, 3), np.float32); inf[:, 1] = np.inf; inf[2, 1] = -np.inf
    out.append(Case("none_inf", inf, np.ones((5, 3), np.float32), found=False))
    out.append(Case("one_pair", s3[:1], d3[:1], found=False))
    # the void rules
    r = np.random.default_rng(31)
    line = (np.array([0.25, -0.125, 2.0]) + r.integers(-64, 65, (40, 1)) / 64 * np.array([0.5, 0.25, 0.5])).astype(np.float32)      # exact in float32
    cloud = np.stack([r.uniform(-1, 1, 40), r.uniform(-1, 1, 40), r.uniform(1, 3, 40)], 1).astype(np.float32)
    out.append(Case("sources_collinear", line, cloud, max_iters=300, found=False))
    out.append(Case("destinations_collinear", cloud, line, max_iters=300, found=False))
    # usable counts straddling the wave, the compaction's run, the scoring stage, and two chunks
    for cnt in sorted({63, 64, 65, run - 1, run, run + 1, stage - 1, stage, stage + 1, 2 * stage + 1}):
        out.append(_truth_case("usable_%d" % cnt, cnt, 0.2, 10 + cnt, extra=max(9, cnt // 16), max_iters=256))
    # the four sigmas of the recovery bounds
    for k, s in enumerate(SIGMAS):
        out.append(_truth_case("noise_sigma_%d" % k, 400, 0.3, 40 + k, sigma=s))
    # the search
    src, dst, label = pairs(600, [MOTION_1, MOTION_2], [60, 40], SIGMA, 0.0, 21)
    out.append(Case("two_motions_60_40", src, dst, threshold=T, truth=MOTION_1, good=label == 0, sigma=SIGMA))
    src, dst, label = pairs(150, [MOTION_1], [1], SIGMA, 0.3, 22)
    out.append(Case("set_twice", np.concatenate([src, src]), np.concatenate([dst, dst]), threshold=T, max_iters=256, truth=MOTION_1,
                    good=np.concatenate([label, label]) == 0, gross=np.concatenate([label, label]) == -1, sigma=SIGMA))
    out.append(_truth_case("outliers_50_stops_early", 400, 0.5, 23, max_iters=2000))
    out.append(_truth_case("outliers_90_cut_at_44", 600, 0.9, 24, max_iters=300, seed=SEED_90))
    out.append(_truth_case("five_hypotheses", 200, 0.0, 25, max_iters=5))
    src, dst, label = pairs(300, [MOTION_1], [1], SIGMA, 0.8, 26)
    out.append(Case("iters_256", src, dst, threshold=T, max_iters=256))
    out.append(Case("iters_257", src, dst, threshold=T, max_iters=257))
    # the two metrics
    src, dst = _near_far(27)
    out.append(Case("near_far_euclid", src, dst, threshold=0.02, max_iters=256))
    out.append(Case("near_far_disparity", src, dst, metric=DISPARITY, threshold=1.0, camera=CAMERA, max_iters=256))
    src, dst, label = pairs(200, [MOTION_1], [1], SIGMA, 0.2, 28)
    src, dst = src.copy(), dst.copy()
    dst[5::7, 2] = -dst[5::7, 2]; dst[3::11, 2] = 0.0; src[2::13] = -src[2::13]          # q_z < 0, q_z == 0, and sources that land behind the camera
    out.append(Case("disparity_z_not_positive", src, dst, metric=DISPARITY, threshold=2.0, camera=CAMERA, max_iters=256))
    src, dst, _ = pairs(300, [MOTION_1], [1], SIGMA, 0.0, 29)
    out.append(Case("mirrored", src, dst * np.array([-1, 1, 1], np.float32), threshold=T, max_iters=512, found=None))
    # tracks into two images
    out.append(_track_case("tracks_33x17", 33, 17, 120, 5, 2, 1, max_iters=256))
    out.append(_track_case("tracks_257x9", 257, 9, 300, 0, 7, 2, max_iters=256))
    out.append(_track_case("tracks_disparity", 33, 17, 100, 1, 0, 3, metric=DISPARITY, threshold=3.0, camera=CAMERA, max_iters=256))
    return out


SEED_90 = 6          # under it (the best index, 298, lies in the cut second round) the statement finds the motion among 300 hypotheses at 90 % outliers (asserted in test_rigid_statement.py)
CASES = _cases()
IDS = [c.id for c in CASES]
BY_ID = {c.id: c for c in CASES}
TRACK_CASES = [c for c in CASES if c.tracks is not None]


@functools.lru_cache(maxsize=None)
def stated(cid, order="index"):
    """the statement's answer for a case, computed once"""
    c = BY_ID[cid]
    return R.fit(c.src, c.dst, order=order, **c.kw())


# ---- a synthetic rig: one plane-and-box scene, moved by a known motion, seen as two disparity images ----------------------------------------
# StereoRig.ego_motion is checked on it (tests/test_gpu_rigid_py.py).  Everything here is host arithmetic: the rig's rectified
# constants come from stereo_rectify (host float64) and the points from vp_reproject_to_3d_host, whose bits are the device's.  The
# scene's noise is not a sigma the generator sets - it is the disparity's sixteenths and the nearest-pixel sampling of the track ends -
# so the recovery bound is not a ratio per sigma: it is the statement's own error on this scene, measured once and written down,
# and the suites assert twice that (one seed is one draw).  tests/test_rigid_statement.py measures both figures again.
EGO_W, EGO_H = 96, 64
EGO_CALIBRATION = dict(K1=np.array([[112.3, 0, 47.4], [0, 111.1, 31.9], [0, 0, 1.0]]), d1=[-0.28, 0.09, 0.0005, -0.0003, -0.013],
                       K2=np.array([[109.8, 0, 48.7], [0, 110.4, 30.2], [0, 0, 1.0]]), d2=[-0.27, 0.08, -0.0004, 0.0006, -0.012], rvec=[0.01, -0.02, 0.03],
                       T=[-0.12, 0.004, -0.003])
EGO_MOTION = (rotation(0.02, -0.04, 0.03), np.array([0.05, -0.02, 0.08]))
EGO_SEARCH = dict(max_iters=512, seed=2)
EGO_MEASURED_ROT = 0.0008067585111682889         # radians: the statement's refit against EGO_MOTION, disparity metric, threshold 1 px
EGO_MEASURED_T = 0.0005964930332446834           # metres
EGO_BOUND_ROT, EGO_BOUND_T = 2 * EGO_MEASURED_ROT, 2 * EGO_MEASURED_T


def _ego_depth(f, cx, cy, Rm, t):
    """(Z (H, W) of the scene moved by (Rm, t) along every pixel's ray, the scene's own coordinates of the point seen there): a slanted
    back plane and a box face in front of it, both given in the scene's frame and intersected analytically"""
    x, y = np.meshgrid(np.arange(EGO_W, dtype=np.float64), np.arange(EGO_H, dtype=np.float64))
    rays = np.stack([(x - cx) / f, (y - cy) / f, np.ones_like(x)], 2)
    best_z, best_p = np.full((EGO_H, EGO_W), np.inf), np.zeros((EGO_H, EGO_W, 3))
    for n, d, inside in ((np.array([0.1, -0.05, -1.0]), 2.0, lambda p: np.ones(p.shape[:2], bool)),
                         (np.array([-0.2, 0.1, -1.0]), 1.2, lambda p: (np.abs(p[..., 0] - 0.1) < 0.3) & (np.abs(p[..., 1]) < 0.2))):
        # scene plane n.p + d = 0; a camera point c = Rm p + t, so n.(Rm^T (c - t)) + d = 0 with c = z ray
        nn = Rm @ n
        z = (nn @ t - d) / (rays @ nn)
        p = (z[..., None] * rays - t) @ Rm
        ok = (z > 0) & inside(p) & (z < best_z)
        best_z[ok], best_p[ok] = z[ok], p[ok]
    return best_z, best_p


@functools.lru_cache(maxsize=None)
def ego_scene():
    """dict: focal_px, cx, cy, baseline_m, Q of the rectified rig; disp (two int16 images, sixteenths of a pixel); prev, next (400, 2)
    float32 and status (400,) bool - the tracks come from the geometry: where the scene point seen at a pixel of frame 0 lands in
    frame 1, if the same surface is visible there; rows: the tracks as vp_lk_flow_dev leaves them"""
    from vision.utils import stereo
    c = EGO_CALIBRATION
    _, _, P1, P2, Q, _, _ = stereo.stereo_rectify(c["K1"], c["d1"], c["K2"], c["d2"], (EGO_W, EGO_H), stereo.rodrigues(c["rvec"]), c["T"], True, 0, (EGO_W, EGO_H))
    f, cx, cy = float(P1[0, 0]), float(P1[0, 2]), float(P1[1, 2])
    b = float(abs(P2[0, 3]) / f)
    Rm, t = EGO_MOTION
    z0, p0 = _ego_depth(f, cx, cy, np.eye(3), np.zeros(3))
    z1, _ = _ego_depth(f, cx, cy, Rm, t)
    disp = [np.rint(f * b / z * 16).astype(np.int16) for z in (z0, z1)]
    r = np.random.default_rng(5)
    px = np.stack([r.integers(0, EGO_W, 400), r.integers(0, EGO_H, 400)], 1)
    c1 = p0[px[:, 1], px[:, 0]] @ Rm.T + t
    nxt = np.stack([f * c1[:, 0] / c1[:, 2] + cx, f * c1[:, 1] / c1[:, 2] + cy], 1).astype(np.float32)
    ix, iy = np.rint(nxt[:, 0]).astype(int), np.rint(nxt[:, 1]).astype(int)
    inside = (ix >= 0) & (ix < EGO_W) & (iy >= 0) & (iy < EGO_H)
    status = inside.copy()
    status[inside] = np.abs(z1[iy[inside], ix[inside]] - c1[inside, 2]) < 0.05          # the same surface, not one in front of it
    rows = np.zeros((400, 4), np.uint32)
    rows[:, :2], rows[:, 3] = nxt.view(np.uint32), status
    return dict(focal_px=f, cx=cx, cy=cy, baseline_m=b, Q=np.ascontiguousarray(Q), disp=disp, prev=px.astype(np.float32), next=nxt, status=status, rows=rows)


@functools.lru_cache(maxsize=None)
def ego_stated():
    """the statement's answer on the scene: the points of both disparity images by vp_reproject_to_3d_host, then R.fit_tracks"""
    from vision import _vp
    from vision.utils import stereo
    s = ego_scene()
    lib = C.CDLL(_vp.LIB_PATH)
    lib.vp_reproject_to_3d_host.restype, lib.vp_reproject_to_3d_host.argtypes = _vp._SIGS["vp_reproject_to_3d_host"]
    pts = []
    for d in s["disp"]:
        xyz = np.zeros((EGO_H, EGO_W, 3), np.float32)
        assert lib.vp_reproject_to_3d_host(d.ctypes.data, 2 * EGO_W, stereo.DISP_I16, EGO_W, EGO_H, s["Q"].ctypes.data, stereo.invalid_disparity(0), xyz.ctypes.data,
                                           12 * EGO_W) == 0
        pts.append(xyz)
    return R.fit_tracks(pts[0], pts[1], s["prev"], s["rows"], metric=DISPARITY, threshold=1.0, camera=(s["focal_px"], s["baseline_m"]), **EGO_SEARCH)


# ---- calling the library --------------------------------------------------------------------------------------------------------------------
CANARY = 0xA5
TAIL = 37            # canary bytes behind the n inlier bytes


def _camera(c, over=None):
    cam = (over or {}).get("camera", c.camera)
    return (0.0, 0.0) if cam is None else cam


def strided(img, pad, fill=-7.5):
    """(buffer (h, row + pad) float32 holding img's rows with `pad` floats of `fill` behind each, stride in bytes)"""
    h = img.shape[0]
    rows = img.reshape(h, -1)
    buf = np.full((h, rows.shape[1] + pad), fill, np.float32)
    buf[:, :rows.shape[1]] = rows
    return buf, buf.strides[0]


def answer(rc, result, counts, inl, c):
    return {"rc": rc, "result": result, "counts": counts.tolist(), "inliers": None if inl is None else inl[:c.n].copy(), "buffer": inl}


def _outputs(c, want_inliers):
    return np.full(31, 7.25), np.full(4, -5, np.int32), (np.full(c.n + TAIL, CANARY, np.uint8) if want_inliers else None)


def call_host(c, want_inliers=True, tracks=None, **over):
    """vp_fit_rigid_host, or vp_fit_rigid_tracks_host for a track case (tracks=False: the array form on the track case's pairs)"""
    lib = library()
    a = dict(c.kw(), **over)
    f, b = _camera(c, over)
    result, counts, inl = _outputs(c, want_inliers)
    ip = None if inl is None else inl.ctypes.data
    if c.tracks is not None and tracks is not False:
        t = c.tracks
        x0, s0 = strided(t["xyz0"], t["pad0"])
        x1, s1 = strided(t["xyz1"], t["pad1"])
        rc = lib.vp_fit_rigid_tracks_host(x0.ctypes.data, s0, x1.ctypes.data, s1, t["w"], t["h"], t["prev"].ctypes.data, t["rows"].ctypes.data, c.n, a["metric"],
                                          a["threshold"], f, b, a["max_iters"], a["confidence"], a["seed"], ip, result.ctypes.data, counts.ctypes.data)
    else:
        rc = lib.vp_fit_rigid_host(c.src.ctypes.data, c.dst.ctypes.data, c.n, a["metric"], a["threshold"], f, b, a["max_iters"], a["confidence"], a["seed"], ip,
                                   result.ctypes.data, counts.ctypes.data)
    return answer(rc, result, counts, inl, c)


def call_f32(ctx, c, want_inliers=True):
    lib = library()
    f, b = _camera(c)
    result, counts, inl = _outputs(c, want_inliers)
    ip = None if inl is None else inl.ctypes.data
    if c.tracks is not None:
        t = c.tracks
        x0, x1 = np.ascontiguousarray(t["xyz0"]), np.ascontiguousarray(t["xyz1"])
        rc = lib.vp_fit_rigid_tracks_f32(ctx, x0.ctypes.data, x1.ctypes.data, t["w"], t["h"], t["prev"].ctypes.data, t["rows"].ctypes.data, c.n, c.metric, c.threshold, f,
                                         b, c.max_iters, c.confidence, c.seed, ip, result.ctypes.data, counts.ctypes.data)
    else:
        rc = lib.vp_fit_rigid_f32(ctx, c.src.ctypes.data, c.dst.ctypes.data, c.n, c.metric, c.threshold, f, b, c.max_iters, c.confidence, c.seed, ip,
                                  result.ctypes.data, counts.ctypes.data)
    return answer(rc, result, counts, inl, c)


def call_dev(vp, c, want_inliers=True):
    """vp_fit_rigid_dev / vp_fit_rigid_tracks_dev on device buffers; the whole inlier buffer comes back, its canary tail included"""
    lib, ctx = library(), vp.default_context().handle
    f, b = _camera(c)
    result, counts, inl = _outputs(c, want_inliers)
    held = []

    def up(a):
        if a is None:
            return None
        p = C.c_void_p()
        vp.check(vp.lib().vp_dev_alloc(ctx, a.nbytes, C.byref(p)), ctx)
        held.append(p.value)
        vp.check(vp.lib().vp_memcpy_h2d(ctx, p.value, a.ctypes.data, a.nbytes), ctx)
        return p.value

    try:
        di = up(inl)
        if c.tracks is not None:
            t = c.tracks
            x0, s0 = strided(t["xyz0"], t["pad0"])
            x1, s1 = strided(t["xyz1"], t["pad1"])
            rc = lib.vp_fit_rigid_tracks_dev(ctx, up(x0), s0, up(x1), s1, t["w"], t["h"], t["prev"].ctypes.data, up(t["rows"]), c.n, c.metric, c.threshold, f, b,
                                             c.max_iters, c.confidence, c.seed, di, result.ctypes.data, counts.ctypes.data)
        else:
            rc = lib.vp_fit_rigid_dev(ctx, up(c.src), up(c.dst), c.n, c.metric, c.threshold, f, b, c.max_iters, c.confidence, c.seed, di, result.ctypes.data,
                                      counts.ctypes.data)
        if inl is not None:
            vp.check(vp.lib().vp_memcpy_d2h(ctx, inl.ctypes.data, di, inl.nbytes), ctx)
    finally:
        for p in held:
            vp.lib().vp_dev_free(ctx, p)
    return answer(rc, result, counts, inl, c)


# ---- comparing ------------------------------------------------------------------------------------------------------------------------------
def rot_angle(A, B):
    """the angle of the rotation that carries B onto A, exact for small angles"""
    D = np.asarray(A, np.float64).reshape(3, 3) @ np.asarray(B, np.float64).reshape(3, 3).T
    v = np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return math.atan2(float(np.linalg.norm(v)) / 2.0, (float(np.trace(D)) - 1.0) / 2.0)


def refit_differences(a, b):
    """(angle between the rotations, |dt| / max(1, |t|), the larger |dcentroid|, |drms|) of two results of 31"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (rot_angle(a[0:9], b[0:9]), float(np.linalg.norm(a[9:12] - b[9:12])) / max(1.0, float(np.linalg.norm(b[9:12]))),
            max(float(np.linalg.norm(a[24:27] - b[24:27])), float(np.linalg.norm(a[27:30] - b[27:30]))), abs(a[30] - b[30]))


def recovery(result, truth):
    """(refit angle, refit |dt|, hypothesis angle, hypothesis |dt|) of a result of 31 against the generating motion"""
    r = np.asarray(result, np.float64)
    Rt, tt = truth
    return (rot_angle(r[0:9], Rt), float(np.linalg.norm(r[9:12] - tt)), rot_angle(r[12:21], Rt), float(np.linalg.norm(r[21:24] - tt)))


def _floor(value, tol):
    return max(tol, 16 * float(np.spacing(abs(value))))


def same_exact(got, want, what):
    """the part that is bit for bit: the best hypothesis, its index, the three counts, the inlier bytes"""
    assert got["rc"] == 0, what
    assert got["counts"] == [want["n_usable"], want["n_inliers"], want["n_hypotheses"], want["best_j"]], (what, got["counts"])
    assert np.array_equal(R.bits(got["result"][12:24]), R.bits(want["result"][12:24])), what + ": the best hypothesis"
    if got["inliers"] is not None:
        assert np.array_equal(got["inliers"], want["inliers"]), what + ": the inlier bytes"
        assert (got["buffer"][len(got["inliers"]):] == CANARY).all(), what + ": a byte behind the inlier bytes was written"
    if not want["found"]:
        assert not got["result"].any(), what


def same_refit(got, want, what):
    if not want["found"]:
        return
    da, dt, dc, dr = refit_differences(got["result"], want["result"])
    w = np.asarray(want["result"], np.float64)
    assert da <= _floor(1.0, TOL_ROT), (what, "rotation", da)
    assert dt <= _floor(max(1.0, float(np.linalg.norm(w[9:12]))), TOL_T), (what, "t", dt)
    assert dc <= _floor(max(float(np.linalg.norm(w[24:27])), float(np.linalg.norm(w[27:30]))), TOL_CENTROID), (what, "centroid", dc)
    assert dr <= _floor(w[30], TOL_RMS), (what, "rms", dr)
