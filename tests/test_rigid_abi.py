"""CPU suite of robust rigid motion: the surface - symbols exported, declared and bound alike, the units
built; every refusal from the arguments alone, which leaves the results untouched; the plan; and the whole algorithm, which
vp_fit_rigid_host, vp_fit_rigid_tracks_host, vp_rigid_hypothesis and vp_rigid_refit run without a device, against the statement
tests/rigid_restate.py."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import rigid_cases as K
import rigid_restate as R
from abi_header import _header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc")
NEW = ["vp_fit_rigid_plan", "vp_fit_rigid_dev", "vp_fit_rigid_f32", "vp_fit_rigid_host", "vp_fit_rigid_tracks_dev", "vp_fit_rigid_tracks_f32",
       "vp_fit_rigid_tracks_host", "vp_rigid_hypothesis", "vp_rigid_refit"]


def test_rigid_symbols_are_exported_declared_and_bound_alike():
    from vision import _vp
    protos = _header_prototypes()
    lib = C.CDLL(_vp.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name) and name in protos and name in _vp._SIGS, name
        assert protos[name][0] == "int" and protos[name][1] == _vp._SIGS[name][1] and _vp._SIGS[name][0] is C.c_int, name
    assert [len(protos[n][1]) for n in NEW] == [3, 14, 14, 13, 20, 18, 19, 7, 5]
    built = open(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "build.py")).read()
    for src in ("vp_rigid.hip", "vp_api_rigid.hip"):
        assert f'"{src}"' in built and os.path.exists(os.path.join(CSRC, src)), src
    header = open(os.path.join(ROOT, "include", "vp.h")).read()
    assert "VP_RIGID_EUCLID = 0, VP_RIGID_DISPARITY = 1" in header and "#define VP_RIGID_RESULT 31" in header and "#define VP_RIGID_COUNTS 4" in header
    assert (_vp.RIGID_EUCLID, _vp.RIGID_DISPARITY, _vp.RIGID_RESULT, _vp.RIGID_COUNTS) == (R.EUCLID, R.DISPARITY, 31, 4)
    kernel = open(os.path.join(CSRC, "vp_rigid.hip")).read()
    assert '#include "vp_rigid_plan.h"' in kernel and "vp_rg_hypothesis" in kernel and "vp_rg_inlier" in kernel and "vp_pl_stop" in kernel
    for unit in ("vp_rigid.hip", "vp_plane.hip", "vp_model.hip"):
        assert '#include "vp_ransac_dev.h"' in open(os.path.join(CSRC, unit)).read(), "the scan and the key reduction are shared, not pasted"
    assert '#include "vp_plane_plan.h"' in open(os.path.join(CSRC, "vp_rigid_plan.h")).read(), "the point test and the stop rule are the plane's"


def test_python_names_and_signatures():
    from vision.utils import stereo
    sig = lambda fn: [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    search = [("threshold", 0.02), ("max_iters", 1000), ("confidence", 0.99), ("seed", 0), ("camera", None), ("return_mask", False)]
    assert sig(stereo.fit_rigid) == [("src", E), ("dst", E)] + search
    assert sig(stereo.rigid_from_tracks) == [("points_prev", E), ("points_cur", E), ("prev_pts", E), ("next_pts", E), ("status", None)] + search
    assert sig(stereo.StereoRig.ego_motion) == [("self", E), ("disp_prev", E), ("disp_cur", E), ("prev_pts", E), ("next_pts", E), ("status", None), ("space", "disparity"),
                                                ("threshold", None), ("min_disparity", 0), ("search", E)]
    assert [f.name for f in __import__("dataclasses").fields(stereo.RigidFit)] == ["found", "R", "t", "hypothesis", "n_usable", "n_inliers", "n_hypotheses", "best_index",
                                                                                  "centroids", "rms", "mask"]
    Rm, t = K.MOTION_2
    fit = stereo.RigidFit(True, Rm, t, np.zeros((3, 4)), 9, 9, 1, 0, np.array([[1.0, 2, 3], [4, 5, 6]]), 0.0)
    assert fit.matrix.shape == (4, 4) and np.array_equal(fit.matrix[:3, :3], Rm) and np.array_equal(fit.matrix[:3, 3], t) and fit.matrix[3].tolist() == [0, 0, 0, 1]
    assert np.abs(fit.inverse().matrix @ fit.matrix - np.eye(4)).max() <= 1e-12 and np.array_equal(fit.inverse().centroids, fit.centroids[::-1])
    from vision import cv2_facade as f
    assert not any(hasattr(f.install(), name) for name in ("estimateAffine3D", "fit_rigid", "solvePnP")), "cv2 has no such operator; estimateAffine3D is another model"


def test_python_operators_refuse_bad_arguments_without_a_context(monkeypatch):
    from vision import _vp
    from vision.utils import stereo

    def no_context(*a, **k):
        raise AssertionError("a context was asked for")
    monkeypatch.setattr(_vp, "default_context", no_context)
    p = np.ones((4, 3), np.float32)
    for bad, words in ((dict(threshold=0.0), "threshold"), (dict(threshold=float("nan")), "threshold"), (dict(max_iters=0), "max_iters"),
                       (dict(max_iters=65537), "max_iters"), (dict(confidence=1.0), "confidence"), (dict(confidence=0.0), "confidence"),
                       (dict(camera=(0.0, 0.1)), "focal_px"), (dict(camera=(500.0, float("inf"))), "baseline"), (dict(camera=(1.0,)), "camera"),
                       (dict(seed=-1), "seed")):
        with pytest.raises(ValueError, match=words):
            stereo.fit_rigid(p, p, **bad)
        with pytest.raises(ValueError, match=words):
            stereo.rigid_from_tracks(np.ones((4, 5, 3), np.float32), np.ones((4, 5, 3), np.float32), np.zeros((3, 2)), np.zeros((3, 2)), **bad)
    with pytest.raises(TypeError):
        stereo.fit_rigid(p.astype(np.float64), p)
    with pytest.raises(TypeError):
        stereo.fit_rigid(p, np.ones((4, 2), np.float32))
    with pytest.raises(ValueError, match="pairs"):
        stereo.fit_rigid(p, p[:3])
    with pytest.raises(ValueError, match="pairs"):
        stereo.fit_rigid(p[:0], p[:0])
    img = np.ones((4, 5, 3), np.float32)
    with pytest.raises(TypeError):
        stereo.rigid_from_tracks(img[:, :, :2], img, np.zeros((3, 2)), np.zeros((3, 2)))
    with pytest.raises(ValueError, match="one size"):
        stereo.rigid_from_tracks(img, img[:3], np.zeros((3, 2)), np.zeros((3, 2)))
    with pytest.raises(ValueError, match="tracks"):
        stereo.rigid_from_tracks(img, img, np.zeros((3, 2)), np.zeros((4, 2)))
    with pytest.raises(ValueError, match="status"):
        stereo.rigid_from_tracks(img, img, np.zeros((3, 2)), np.zeros((3, 2)), status=np.ones(2))
    rig = object.__new__(stereo.StereoRig)
    rig.focal_px, rig.baseline_m = 100.0, 0.1
    d = np.zeros((4, 5), np.int16)
    with pytest.raises(ValueError, match="space"):
        rig.ego_motion(d, d, np.zeros((3, 2)), np.zeros((3, 2)), space="pixels")
    with pytest.raises(ValueError, match="threshold"):
        rig.ego_motion(d, d, np.zeros((3, 2)), np.zeros((3, 2)), threshold=-1.0)
    with pytest.raises(ValueError, match="tracks"):
        rig.ego_motion(d, d, np.zeros((3, 2)), np.zeros((2, 2)))


# ---- the algorithm ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.CASES, ids=K.IDS)
def test_host_fit_is_the_statements(case):
    want = K.stated(case.id)
    got = K.call_host(case)
    K.same_exact(got, want, case.id)
    K.same_refit(got, want, case.id)
    K.same_exact(K.call_host(case, want_inliers=False), want, case.id)
    if case.tracks is not None:                 # the array form on the pairs the tracks give: the same search
        arr = K.call_host(case, tracks=False)
        K.same_exact(arr, want, case.id + " as arrays")
        assert np.array_equal(R.bits(arr["result"]), R.bits(got["result"]))


@pytest.mark.parametrize("cid", ["sources_collinear", "set_twice", "usable_65"])
def test_single_hypotheses(cid):
    lib, c = K.library(), K.BY_ID[cid]
    P, Q, _ = R.pairs_of(c.src, c.dst)
    voids = 0
    for j in range(512):
        s, m = R.hypothesis(P, Q, c.seed, j)
        s3, motion = np.full(3, -9, np.int32), np.full(12, 7.25)
        rc = lib.vp_rigid_hypothesis(P.ctypes.data, Q.ctypes.data, len(P), c.seed, j, s3.ctypes.data, motion.ctypes.data)
        assert rc == (0 if m is None else 1) and s3.tolist() == s
        assert np.array_equal(R.bits(motion), R.bits([0.0] * 12 if m is None else m)), (cid, j)
        voids += m is None
    assert (voids == 512) == (cid == "sources_collinear") and (voids > 0) == (cid != "usable_65")


def test_refit_alone_is_the_statements():
    lib = K.library()
    for c in K.CASES:
        w = K.stated(c.id)
        if not w["found"]:
            continue
        P, Q, idx = R.pairs_of(c.src, c.dst)
        keep = np.ascontiguousarray(w["inliers"][idx])
        for k in (keep, None):
            want = R.refit(P, Q, k)
            got = np.full(31, 7.25)
            rc = lib.vp_rigid_refit(P.ctypes.data, Q.ctypes.data, len(P), None if k is None else k.ctypes.data, got.ctypes.data)
            assert rc == (want is not None), c.id
            if want is None:
                assert not got.any()
                continue
            K.same_refit({"result": got}, {"found": True, "result": want}, c.id)
    line = np.array([[0, 0, 1], [1, 1, 2], [2, 2, 3], [3, 3, 4]], np.float32)
    got = np.full(31, 7.25)
    assert lib.vp_rigid_refit(line.ctypes.data, line.ctypes.data, 4, None, got.ctypes.data) == 0 and not got.any()


# ---- refusals and the plan -------------------------------------------------------------------------------------------------------------
nan, inf = float("nan"), float("inf")
_SEARCH_ROWS = [("metric", dict(metric=2), "metric"), ("metric_neg", dict(metric=-1), "metric"),
                ("threshold0", dict(threshold=0.0), "threshold"), ("threshold_nan", dict(threshold=nan), "threshold"), ("threshold_inf", dict(threshold=inf), "threshold"),
                ("focal0", dict(f=0.0), "focal_px"), ("focal_nan", dict(f=nan), "focal_px"), ("focal_inf", dict(f=inf), "focal_px"),
                ("baseline0", dict(b=0.0), "baseline"), ("baseline_neg", dict(b=-0.1), "baseline"), ("baseline_nan", dict(b=nan), "baseline"),
                ("iters0", dict(max_iters=0), "max_iters"), ("iters_many", dict(max_iters=65537), "max_iters"),
                ("conf0", dict(confidence=0.0), "confidence"), ("conf1", dict(confidence=1.0), "confidence"), ("conf_nan", dict(confidence=nan), "confidence")]


def _array_refusals():
    c = K.BY_ID["usable_65"]
    src, dst = c.src.copy(), c.dst.copy()
    inl = np.full(c.n + K.TAIL, K.CANARY, np.uint8)
    base = dict(src=src.ctypes.data, dst=dst.ctypes.data, n=c.n, metric=1, threshold=1.0, f=500.0, b=0.1, max_iters=100, confidence=0.99, inl=inl.ctypes.data,
                result=True, counts=True)
    rows = [("src", dict(src=None), "pointer"), ("dst", dict(dst=None), "pointer"), ("result", dict(result=False), "pointer"), ("counts", dict(counts=False), "pointer"),
            ("n0", dict(n=0), "1 to 1048576"), ("n_neg", dict(n=-3), "1 to 1048576"), ("n_many", dict(n=2 ** 20 + 1), "1 to 1048576"),
            ("src_misaligned", dict(src=src.ctypes.data + 2), "aligned"), ("dst_misaligned", dict(dst=dst.ctypes.data + 1), "aligned"),
            ("overlap_src", dict(inl=src.ctypes.data + 8), "overlap"), ("overlap_dst", dict(inl=dst.ctypes.data + c.n * 12 - 1), "overlap")] + _SEARCH_ROWS
    return base, rows, (src, dst, inl)


def _track_refusals():
    c = K.BY_ID["tracks_33x17"]
    t = c.tracks
    x0, s0 = K.strided(t["xyz0"], t["pad0"])
    x1, s1 = K.strided(t["xyz1"], t["pad1"])
    prev, rows_ = t["prev"].copy(), t["rows"].copy()
    inl = np.full(c.n + K.TAIL, K.CANARY, np.uint8)
    w, h = t["w"], t["h"]
    base = dict(x0=x0.ctypes.data, s0=s0, x1=x1.ctypes.data, s1=s1, w=w, h=h, prev=prev.ctypes.data, rows=rows_.ctypes.data, n=c.n, metric=1, threshold=1.0, f=500.0,
                b=0.1, max_iters=100, confidence=0.99, inl=inl.ctypes.data, result=True, counts=True)
    rows = [("xyz_prev", dict(x0=None), "pointer"), ("xyz_cur", dict(x1=None), "pointer"), ("prev_pts", dict(prev=None), "pointer"), ("tracks", dict(rows=None), "pointer"),
            ("result", dict(result=False), "pointer"), ("counts", dict(counts=False), "pointer"),
            ("n0", dict(n=0), "1 to 1048576"), ("n_many", dict(n=2 ** 20 + 1), "1 to 1048576"),
            ("w0", dict(w=0), "1 to 4096"), ("w4097", dict(w=4097), "1 to 4096"), ("h0", dict(h=0), "1 to 4096"), ("h4097", dict(h=4097), "1 to 4096"),
            ("stride_prev", dict(s0=w * 12 - 4), "stride is below"), ("stride_cur", dict(s1=w * 12 - 4), "stride is below"),
            ("stride_prev_odd", dict(s0=s0 + 2), "multiple of 4"), ("stride_cur_odd", dict(s1=w * 12 + 2), "multiple of 4"),
            ("xyz_misaligned", dict(x1=x1.ctypes.data + 2), "aligned"), ("tracks_misaligned", dict(rows=rows_.ctypes.data + 2), "aligned"),
            ("overlap_prev", dict(inl=x0.ctypes.data + 8), "overlap"), ("overlap_cur", dict(inl=x1.ctypes.data + 8), "overlap"),
            ("overlap_tracks", dict(inl=rows_.ctypes.data + 5), "overlap"), ("overlap_prev_pts", dict(inl=prev.ctypes.data + c.n * 8 - 1), "overlap prev_pts")] + _SEARCH_ROWS
    return base, rows, (x0, x1, prev, rows_, inl)


_ABASE, _AROWS, _AKEEP = _array_refusals()
_TBASE, _TROWS, _TKEEP = _track_refusals()
# Every entry refuses from its arguments alone, before it looks at its context: the device and staging forms are driven here with a
# NULL context and host addresses, which a refusal never reads.  The packed _f32 track form has no strides to refuse, and prev_pts
# and the inlier bytes share an address space only where both are host memory.
_ENTRIES = ("host", "dev", "f32")
_ACOMBOS = [(e, r) for e in _ENTRIES for r in _AROWS]
_TCOMBOS = [(e, r) for e in _ENTRIES for r in _TROWS if not (e == "f32" and r[0].startswith("stride_")) and not (e == "dev" and r[0] == "overlap_prev_pts")]


def _untouched(before, now):
    for b, a in zip(before, now):
        assert np.array_equal(b.view(np.uint8), a.view(np.uint8))


@pytest.mark.parametrize("entry,row", _ACOMBOS, ids=["%s-%s" % (e, r[0]) for e, r in _ACOMBOS])
def test_array_refusals_leave_everything_untouched(entry, row):
    _, change, words = row
    a = dict(_ABASE, **change)
    before = [b.copy() for b in _AKEEP]
    result, counts = np.full(31, 7.25), np.full(4, -5, np.int32)
    lib = K.library()
    args = (a["src"], a["dst"], a["n"], a["metric"], a["threshold"], a["f"], a["b"], a["max_iters"], a["confidence"], 0, a["inl"],
            result.ctypes.data if a["result"] else None, counts.ctypes.data if a["counts"] else None)
    rc = lib.vp_fit_rigid_host(*args) if entry == "host" else getattr(lib, "vp_fit_rigid_" + entry)(None, *args)
    assert rc == -1 and words in lib.vp_last_error(None).decode(), lib.vp_last_error(None).decode()
    assert (result == 7.25).all() and (counts == -5).all() and (_AKEEP[2] == K.CANARY).all()
    _untouched(before, _AKEEP)


@pytest.mark.parametrize("entry,row", _TCOMBOS, ids=["%s-%s" % (e, r[0]) for e, r in _TCOMBOS])
def test_track_refusals_leave_everything_untouched(entry, row):
    _, change, words = row
    a = dict(_TBASE, **change)
    before = [b.copy() for b in _TKEEP]
    result, counts = np.full(31, 7.25), np.full(4, -5, np.int32)
    lib = K.library()
    images = (a["x0"], a["x1"]) if entry == "f32" else (a["x0"], a["s0"], a["x1"], a["s1"])
    args = images + (a["w"], a["h"], a["prev"], a["rows"], a["n"], a["metric"], a["threshold"], a["f"], a["b"], a["max_iters"], a["confidence"], 0, a["inl"],
                     result.ctypes.data if a["result"] else None, counts.ctypes.data if a["counts"] else None)
    rc = lib.vp_fit_rigid_tracks_host(*args) if entry == "host" else getattr(lib, "vp_fit_rigid_tracks_" + entry)(None, *args)
    assert rc == -1 and words in lib.vp_last_error(None).decode(), lib.vp_last_error(None).decode()
    assert (result == 7.25).all() and (counts == -5).all() and (_TKEEP[4] == K.CANARY).all()
    _untouched(before, _TKEEP)


def test_the_camera_counts_under_the_disparity_metric_only():
    c = K.BY_ID["usable_65"]
    got = K.call_host(c, camera=(nan, -1.0))
    K.same_exact(got, K.stated(c.id), "euclid ignores focal_px and baseline")


def test_hypothesis_and_refit_refusals():
    lib = K.library()
    p, s3, m = np.ones((4, 3), np.float32), np.full(3, -9, np.int32), np.full(12, 7.25)
    P, S, Mo = p.ctypes.data, s3.ctypes.data, m.ctypes.data
    for args, words in (((None, P, 4, 0, 0, S, Mo), "pointer"), ((P, None, 4, 0, 0, S, Mo), "pointer"), ((P, P, 4, 0, 0, None, Mo), "pointer"),
                        ((P, P, 4, 0, -1, S, Mo), "0 to 65535"), ((P, P, 4, 0, 65536, S, Mo), "0 to 65535"), ((P, P, -1, 0, 0, S, Mo), "pairs"),
                        ((P, P, 2 ** 20 + 1, 0, 0, S, Mo), "pairs")):
        assert lib.vp_rigid_hypothesis(*args) < 0 and words in lib.vp_last_error(None).decode()
        assert (s3 == -9).all() and (m == 7.25).all()
    res = np.full(31, 7.25)
    assert lib.vp_rigid_refit(None, P, 4, None, res.ctypes.data) < 0 and lib.vp_rigid_refit(P, P, -1, None, res.ctypes.data) < 0 and (res == 7.25).all()


def test_plan_geometry_is_consistent_with_the_workspace():
    lib = K.library()
    ws, g = C.c_size_t(0), np.zeros(8, np.int32)
    assert lib.vp_fit_rigid_plan(0, C.addressof(ws), g.ctypes.data) != 0 and lib.vp_fit_rigid_plan(4, None, g.ctypes.data) != 0
    assert lib.vp_fit_rigid_plan(2 ** 20 + 1, C.addressof(ws), g.ctypes.data) != 0
    al = lambda v: (v + 255) // 256 * 256
    for n in (1, 65, 1024, 1025, 100000, 2 ** 20):
        bytes_, g = K.geometry(n)
        run, stage, per_block, threads, rnd, n_, runs, chunks = (int(v) for v in g)
        assert n_ == n and runs == -(-n // run) and chunks == -(-n // stage)
        assert run % threads == 0 and threads % 64 == 0 and rnd == R.ROUND and rnd % per_block == 0 and stage * 32 <= 32768 and chunks <= 65535
        rounds = 65536 // rnd
        sizes = [n * 32, runs * 4, runs * 4, rounds * 8, rnd * 4, rnd * 4, rnd * 18 * 8]
        state = 6 * 4 + (18 + 17) * 8           # the words, the best hypothesis, the refit sums
        assert bytes_ == sum(al(s) for s in sizes) + state
