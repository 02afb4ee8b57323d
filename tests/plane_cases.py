"""The cases shared by the plane-fitting suites (tests/test_plane_statement.py, test_plane_abi.py, test_gpu_plane.py,
test_gpu_plane_py.py): small XYZ images from seeded generators, each with its box, mask, metric, threshold, seed, max_iters and
confidence; the statement's answer per case, computed once; one caller for the three image entries of libvp; and the refit
tolerance, which is measured on the statement alone."""
import ctypes as C
import functools
import math

import numpy as np

import plane_restate as R

PERP, ALONG_Z = R.PERP, R.ALONG_Z

# ---- the refit tolerance -------------------------------------------------------------------------------------------------------------------
# The device adds the ten refit sums in a free order, so the refit is compared within a tolerance.  It is measured on the statement:
# for every case the restatement's refit runs with its sums in index order, reversed and pairwise; SPREAD is the largest difference,
# over the cases, of the angle between the normals, |d' - d| / max(1, |d|), |centroid' - centroid| and |rms' - rms|; the tolerance is
# 64 times the spread (the device groups by waves and blocks, not by pairs).  tests/test_plane_statement.py measures the spreads
# again and compares them with these constants.
SPREAD_ANGLE = 4.2616323385626885e-15
SPREAD_D = 4.241177318975032e-15
SPREAD_CENTROID = 0.0            # the floor applies: 16 ulp of the centroid's length
SPREAD_RMS = 1.557174528210581e-13
TOL_ANGLE, TOL_D, TOL_CENTROID, TOL_RMS = 64 * SPREAD_ANGLE, 64 * SPREAD_D, 64 * SPREAD_CENTROID, 64 * SPREAD_RMS


def library():
    from vision import _vp
    lib = C.CDLL(_vp.LIB_PATH)
    for name, (res, args) in _vp._SIGS.items():
        if name.startswith(("vp_fit_plane_", "vp_plane_", "vp_model_stop_table")) or name == "vp_last_error":
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


@functools.lru_cache(maxsize=None)
def geometry(w=64, h=64, box=None):
    """(workspace bytes, geometry[8]) of vp_fit_plane_plan"""
    ws, g = C.c_size_t(0), np.zeros(8, np.int32)
    b = None if box is None else np.array(box, np.int32)
    rc = library().vp_fit_plane_plan(w, h, None if b is None else b.ctypes.data, C.addressof(ws), g.ctypes.data)
    assert rc == 0
    return ws.value, g


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------
def scene(w, h, planes, shares, sigma, outliers, seed, zsign=1.0):
    """(xyz float32 (h, w, 3), label int (h, w)): every pixel gets a random (X, Y) in [-1, 1]^2; the share shares[i] of the pixels lies on
    planes[i] = (a, b, c): Z = a X + b Y + c with noise along Z uniform in [-2 sigma, 2 sigma]; the share `outliers` has Z uniform in
    [0.3, 4]; label: the plane's number, -1 for an outlier"""
    r = np.random.default_rng(4200 + seed)
    n = w * h
    X, Y = r.uniform(-1, 1, n), r.uniform(-1, 1, n)
    label = np.full(n, -1)
    order = r.permutation(n)
    k_out = int(round(outliers * n))
    rest = order[k_out:]
    cuts = np.round(np.cumsum(shares) / np.sum(shares) * len(rest)).astype(int)
    lo = 0
    for i, hi in enumerate(cuts):
        label[rest[lo:hi]] = i
        lo = hi
    Z = r.uniform(0.3, 4.0, n)
    for i, (a, b, c) in enumerate(planes):
        m = label == i
        Z[m] = a * X[m] + b * Y[m] + c + r.uniform(-2 * sigma, 2 * sigma, m.sum())
    xyz = np.stack([X, Y, zsign * Z], 1).astype(np.float32).reshape(h, w, 3)
    return xyz, label.reshape(h, w)


def plane_of(a, b, c, zsign=1.0):
    """(n0, n1, n2, d) with d > 0 of zsign Z = a X + b Y + c"""
    v = np.array([a, b, -zsign, c], np.float64) / math.sqrt(a * a + b * b + 1.0)
    return v if v[3] > 0 else -v


class Case:
    def __init__(self, cid, xyz, box=None, mask=None, metric=PERP, threshold=0.02, seed=0, max_iters=512, confidence=0.99, xyz_pad=0, mask_pad=0, inl_pad=0,
                 truth=None, good=None, found=True):
        self.id, self.xyz, self.box, self.mask, self.metric = cid, np.ascontiguousarray(xyz, np.float32), box, mask, metric
        self.threshold, self.seed, self.max_iters, self.confidence = threshold, seed, max_iters, confidence
        self.xyz_pad, self.mask_pad, self.inl_pad = xyz_pad, mask_pad, inl_pad      # floats / bytes / bytes behind each row
        self.truth, self.good, self.found = truth, good, found                       # the generating plane, its pixels, is there a model
        self.xyz.flags.writeable = False
        self.h, self.w = self.xyz.shape[:2]

    def kw(self):
        return dict(box=self.box, mask=self.mask, metric=self.metric, threshold=self.threshold, max_iters=self.max_iters, confidence=self.confidence, seed=self.seed)


def _with_usable(xyz, count, seed):
    """exactly `count` usable pixels: the others, chosen at random, become the three zeros"""
    r = np.random.default_rng(99 + seed)
    flat = xyz.reshape(-1, 3).copy()
    kill = r.permutation(len(flat))[:len(flat) - count]
    flat[kill] = 0.0
    return flat.reshape(xyz.shape)


SIGMA = 0.003
P1, P2 = (0.2, -0.1, 2.0), (-0.3, 0.25, 1.2)


def _cases():
    out = []
    T = 4 * SIGMA

    def planar(cid, w, h, outliers, scene_seed, plane=P1, zsign=1.0, **kw):
        xyz, label = scene(w, h, [plane], [1], SIGMA, outliers, scene_seed, zsign)
        kw.setdefault("threshold", T)
        return Case(cid, xyz, truth=plane_of(*plane, zsign), good=label == 0, **kw), label

    # the smallest inputs
    tri = np.array([[[0.5, 0.1, 2.0], [0, 0, 0], [-0.4, 0.3, 2.2], [0.1, -0.6, 1.9]]], np.float32)
    out.append(Case("three_points", tri, max_iters=256))
    two = tri.copy(); two[0, 2] = 0
    out.append(Case("two_points", two, found=False))
    out.append(Case("none_zeros", np.zeros((3, 5, 3), np.float32), found=False))
    out.append(Case("none_nan", np.full((3, 5, 3), np.nan, np.float32), found=False))
    mixed = np.ones((3, 5, 3), np.float32); mixed[:, :, 1] = np.inf; mixed[1, :, 1] = -np.inf; mixed[0, 0] = (np.nan, 1, np.inf)
    out.append(Case("none_inf", mixed, found=False))
    col = np.array([[[0, 0.5, 2], [0.25, 0.5, 2.25], [1, 0.5, 3], [0.3, -0.7, 1.5]]], np.float32)
    out.append(Case("collinear_plus_one", col, max_iters=256))
    # boxes, strides, masks
    c, _ = planar("box_one_row", 40, 9, 0.2, 1, box=(3, 4, 30, 1)); out.append(c)
    c, _ = planar("box_one_column", 9, 40, 0.2, 2, box=(4, 3, 1, 30)); out.append(c)
    c, _ = planar("box_odd_x0_padded", 67, 5, 0.2, 3, box=(5, 1, 41, 3), xyz_pad=5, inl_pad=3); out.append(c)
    c, _ = planar("mask_cuts_runs", 50, 6, 0.2, 4, mask_pad=7, inl_pad=1)
    m = np.full((6, 50), 200, np.uint8); m[:, 10:13] = 0; m[2] = 0; m[4, ::2] = 0; m[5, 49] = 0
    c.mask = m; out.append(c)
    xyz, label = scene(48, 10, [P1], [1], SIGMA, 0.2, 5)
    xyz[1, 3:9] = np.nan; xyz[6, 40:] = 0
    m = np.zeros((10, 48), np.uint8); m[1:9, 2:45] = 1
    out.append(Case("box_and_mask_and_holes", xyz, box=(1, 0, 46, 9), mask=m, threshold=T, truth=plane_of(*P1), good=label == 0))
    # usable counts straddling the wave, the compaction's run and the scoring stage
    _, g = geometry()
    for S in sorted({64, int(g[0]), int(g[1])}):
        side = (11, 7) if S == 64 else (35, 30)
        for cnt in (S - 1, S, S + 1):
            xyz, label = scene(side[0], side[1], [P1], [1], SIGMA, 0.2, 10 + cnt)
            xyz = _with_usable(xyz, cnt, cnt)
            out.append(Case("usable_%d" % cnt, xyz, threshold=T, max_iters=256, truth=plane_of(*P1), good=(label == 0) & (xyz != 0).any(2)))
    # rank carry across runs: a width of 257, unusable pixels at both ends of each run
    xyz, label = scene(257, 9, [P1], [1], SIGMA, 0.2, 20)
    run = int(g[0])
    flat = xyz.reshape(-1, 3)
    for b in range(0, len(flat) + run, run):
        flat[max(b - 3, 0):b + 3] = 0
    out.append(Case("width_257_run_ends", xyz, threshold=T, max_iters=256, truth=plane_of(*P1), good=(label == 0) & (xyz != 0).any(2)))
    # the search
    xyz, label = scene(40, 30, [P1, P2], [60, 40], SIGMA, 0.0, 21)
    out.append(Case("two_planes_60_40", xyz, threshold=T, truth=plane_of(*P1), good=label == 0))
    xyz, label = scene(24, 10, [P1], [1], SIGMA, 0.3, 22)
    out.append(Case("set_twice", np.concatenate([xyz, xyz]), threshold=T, max_iters=256, truth=plane_of(*P1), good=np.concatenate([label, label]) == 0))
    c, _ = planar("outliers_50_stops_early", 30, 20, 0.5, 23, max_iters=2000); out.append(c)
    c, _ = planar("outliers_90_cut_at_44", 40, 25, 0.9, 24, max_iters=300, seed=SEED_90); out.append(c)
    c, _ = planar("five_hypotheses", 20, 10, 0.0, 25, max_iters=5); out.append(c)
    c, _ = planar("facing_away", 24, 12, 0.2, 26, zsign=-1.0); out.append(c)
    r = np.random.default_rng(27)
    flat = np.concatenate([r.uniform(-1, 1, (60, 2)), np.zeros((60, 1))], 1).astype(np.float32).reshape(6, 10, 3)
    out.append(Case("through_origin", flat, max_iters=300, found=False))
    wall = np.concatenate([np.ones((60, 1)), r.uniform(-1, 1, (60, 1)), r.uniform(1, 3, (60, 1))], 1).astype(np.float32).reshape(6, 10, 3)
    out.append(Case("along_z_vertical_wall", wall, metric=ALONG_Z, max_iters=300, found=False))
    out.append(Case("perp_vertical_wall", wall, metric=PERP, max_iters=256))
    xyz, label = scene(30, 20, [(1.0, 0.0, 2.0)], [1], 0.01, 0.1, 28)
    for metric, name in ((PERP, "slant_45_perp"), (ALONG_Z, "slant_45_along_z")):
        out.append(Case(name, xyz, metric=metric, threshold=0.015, max_iters=256))
    c, _ = planar("along_z_plane", 32, 16, 0.3, 29, metric=ALONG_Z); out.append(c)
    return out


SEED_90 = 22         # under it the statement finds the plane among 300 hypotheses at 90 % outliers (asserted in test_plane_statement.py)
CASES = _cases()
IDS = [c.id for c in CASES]
BY_ID = {c.id: c for c in CASES}


@functools.lru_cache(maxsize=None)
def stated(cid, order="index"):
    """the statement's answer for a case, computed once"""
    c = BY_ID[cid]
    return R.fit(c.xyz, order=order, **c.kw())


# ---- calling the library --------------------------------------------------------------------------------------------------------------------
CANARY = 0xA5


def strided(img, pad, fill):
    """(buffer (h, row + pad) of img's dtype holding img's rows with `pad` elements of `fill` behind each, stride in bytes)"""
    h = img.shape[0]
    rows = img.reshape(h, -1)
    buf = np.full((h, rows.shape[1] + pad), fill, rows.dtype)
    buf[:, :rows.shape[1]] = rows
    return buf, buf.strides[0]


def host_buffers(c, want_inliers=True):
    xyz, xs = strided(c.xyz, c.xyz_pad, np.float32(-7.5))
    mask, ms = (None, 0) if c.mask is None else strided(np.ascontiguousarray(c.mask, np.uint8), c.mask_pad, 1)
    inl, is_ = strided(np.full((c.h, c.w), CANARY, np.uint8), c.inl_pad, CANARY) if want_inliers else (None, 0)
    return xyz, xs, mask, ms, inl, is_


def answer(rc, result, counts, inl, c):
    return {"rc": rc, "result": result, "counts": counts.tolist(), "inliers": None if inl is None else inl[:, :c.w].copy(), "buffer": inl}


def call_host(c, want_inliers=True, **over):
    lib = library()
    xyz, xs, mask, ms, inl, is_ = host_buffers(c, want_inliers)
    box = None if c.box is None else np.array(c.box, np.int32)
    result, counts = np.full(12, 7.25), np.full(4, -5, np.int32)
    a = dict(c.kw(), **over)
    rc = lib.vp_fit_plane_host(xyz.ctypes.data, xs, c.w, c.h, None if box is None else box.ctypes.data, None if mask is None else mask.ctypes.data, ms, a["metric"],
                               a["threshold"], a["max_iters"], a["confidence"], a["seed"], None if inl is None else inl.ctypes.data, is_, result.ctypes.data,
                               counts.ctypes.data)
    return answer(rc, result, counts, inl, c)


def call_f32(ctx, c, want_inliers=True):
    lib = library()
    box = None if c.box is None else np.array(c.box, np.int32)
    mask = None if c.mask is None else np.ascontiguousarray(c.mask, np.uint8)
    inl = np.full((c.h, c.w), CANARY, np.uint8) if want_inliers else None
    result, counts = np.full(12, 7.25), np.full(4, -5, np.int32)
    rc = lib.vp_fit_plane_f32(ctx, c.xyz.ctypes.data, c.w, c.h, None if box is None else box.ctypes.data, None if mask is None else mask.ctypes.data, c.metric,
                              c.threshold, c.max_iters, c.confidence, c.seed, None if inl is None else inl.ctypes.data, result.ctypes.data, counts.ctypes.data)
    return answer(rc, result, counts, inl, c)


def call_dev(vp, c, want_inliers=True):
    """vp_fit_plane_dev on strided device images; the whole inlier buffer comes back, padding included"""
    lib, ctx = library(), vp.default_context().handle
    xyz, xs, mask, ms, inl, is_ = host_buffers(c, want_inliers)
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
        dx, dm, di = up(xyz), up(mask), up(inl)
        box = None if c.box is None else np.array(c.box, np.int32)
        result, counts = np.full(12, 7.25), np.full(4, -5, np.int32)
        rc = lib.vp_fit_plane_dev(ctx, dx, xs, c.w, c.h, None if box is None else box.ctypes.data, dm, ms, c.metric, c.threshold, c.max_iters, c.confidence, c.seed,
                                  di, is_, result.ctypes.data, counts.ctypes.data)
        if inl is not None:
            vp.check(vp.lib().vp_memcpy_d2h(ctx, inl.ctypes.data, di, inl.nbytes), ctx)
    finally:
        for p in held:
            vp.lib().vp_dev_free(ctx, p)
    return answer(rc, result, counts, inl, c)


# ---- comparing ------------------------------------------------------------------------------------------------------------------------------
def angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return math.atan2(float(np.linalg.norm(np.cross(a, b))), float(np.dot(a, b)))


def refit_differences(a, b):
    """(angle between the normals, |dd| / max(1, |d|), |dcentroid|, |drms|) of two results of twelve"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (angle(a[:3], b[:3]), abs(a[3] - b[3]) / max(1.0, abs(b[3])), float(np.linalg.norm(a[8:11] - b[8:11])), abs(a[11] - b[11]))


def _floor(value, tol):
    return max(tol, 16 * float(np.spacing(abs(value))))


def same_exact(got, want, what):
    """the part that is bit for bit: the best hypothesis, its index, the three counts, the inlier image"""
    assert got["rc"] == 0, what
    assert got["counts"] == [want["n_usable"], want["n_inliers"], want["n_hypotheses"], want["best_j"]], what
    assert np.array_equal(R.bits(got["result"][4:8]), R.bits(want["result"][4:8])), what + ": the best hypothesis"
    if got["inliers"] is not None:
        assert np.array_equal(got["inliers"], want["inliers"]), what + ": the inlier image"
    if not want["found"]:
        assert not got["result"].any(), what


def same_refit(got, want, what):
    if not want["found"]:
        return
    da, dd, dc, dr = refit_differences(got["result"], want["result"])
    w = want["result"]
    assert da <= _floor(1.0, TOL_ANGLE), (what, "angle", da)
    assert dd <= _floor(max(1.0, abs(w[3])), TOL_D) / 1.0, (what, "d", dd)
    assert dc <= _floor(float(np.linalg.norm(w[8:11])), TOL_CENTROID), (what, "centroid", dc)
    assert dr <= _floor(w[11], TOL_RMS), (what, "rms", dr)
