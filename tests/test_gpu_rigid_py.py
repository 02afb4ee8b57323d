"""GPU suite of the Python layer of rigid motion (vision.utils.stereo.fit_rigid, rigid_from_tracks, StereoRig.ego_motion; DESIGN.md
section 4.39) against the statement tests/rigid_restate.py and against a synthetic rig whose motion is known."""
import numpy as np
import pytest

import rigid_cases as K
import rigid_restate as R

pytestmark = pytest.mark.gpu


def _same(fit, want, what):
    assert fit.found == want["found"] and (fit.n_usable, fit.n_inliers, fit.n_hypotheses, fit.best_index) == (want["n_usable"], want["n_inliers"], want["n_hypotheses"],
                                                                                                               want["best_j"]), what
    hyp = np.concatenate([fit.hypothesis[:, :3].reshape(-1), fit.hypothesis[:, 3]])
    assert np.array_equal(R.bits(hyp), R.bits(want["result"][12:24])), what
    got = {"result": np.concatenate([fit.R.reshape(-1), fit.t, hyp, fit.centroids.reshape(-1), [fit.rms]])}
    K.same_refit(got, want, what)


def test_fit_rigid_is_the_statements(vp):
    from vision.utils import stereo
    for cid in ("usable_1025", "near_far_disparity", "two_pairs", "disparity_z_not_positive"):
        c, want = K.BY_ID[cid], K.stated(cid)
        kw = dict(threshold=c.threshold, max_iters=c.max_iters, confidence=c.confidence, seed=c.seed, camera=c.camera)
        a = stereo.fit_rigid(c.src, c.dst, return_mask=True, **kw)
        _same(a, want, cid)
        assert a.mask.dtype == np.uint8 and np.array_equal(a.mask, want["inliers"]) and stereo.fit_rigid(c.src, c.dst, **kw).mask is None
        if a.found:
            assert np.abs(a.inverse().matrix @ a.matrix - np.eye(4)).max() <= 1e-12 and abs(np.linalg.det(a.R) - 1) <= 1e-12
            assert np.array_equal(a.matrix[:3, :3], a.R) and np.array_equal(a.matrix[:3, 3], a.t)
        else:
            assert not a.R.any() and not a.t.any() and a.best_index == -1


def test_rigid_from_tracks_numpy_and_device_images_agree(vp):
    from vision.devmat import DeviceMat
    from vision.utils import stereo
    ctx = vp.default_context()
    for c in K.TRACK_CASES:
        want, t = K.stated(c.id), c.tracks
        cur = t["rows"][:, :2].copy().view(np.float32)
        status = (t["rows"][:, 3] != 0).astype(np.uint8)
        kw = dict(threshold=c.threshold, max_iters=c.max_iters, confidence=c.confidence, seed=c.seed, camera=c.camera, return_mask=True)
        fits = [stereo.rigid_from_tracks(t["xyz0"], t["xyz1"], t["prev"], cur, status, **kw),
                stereo.rigid_from_tracks(DeviceMat.from_host(ctx, t["xyz0"]), DeviceMat.from_host(ctx, t["xyz1"]), t["prev"], cur, status, **kw),
                stereo.rigid_from_tracks(t["xyz0"], DeviceMat.from_host(ctx, t["xyz1"]), t["prev"], cur, status, **kw)]
        for f in fits:
            _same(f, want, c.id)
            assert isinstance(f.mask, np.ndarray) and np.array_equal(f.mask, want["inliers"])
        assert np.array_equal(R.bits(fits[1].hypothesis), R.bits(fits[0].hypothesis)) and np.array_equal(fits[1].mask, fits[0].mask)


# ---- the synthetic rig of rigid_cases.ego_scene: one plane-and-box scene, moved by a known motion, seen as two disparity images -------------
@pytest.fixture(scope="module")
def rig(vp):
    from vision.utils import stereo
    c = K.EGO_CALIBRATION
    return stereo.StereoRig(c["K1"], c["d1"], c["K2"], c["d2"], (K.EGO_W, K.EGO_H), stereo.rodrigues(c["rvec"]), c["T"])


def test_ego_motion_recovers_a_known_motion(vp, rig):
    """Recovery within the statement's measured bounds: rigid_cases.EGO_BOUND_* are twice what the statement itself leaves of the
    motion on this scene (measured on the CPU by tests/test_rigid_statement.py)."""
    from vision.devmat import DeviceMat
    s, want = K.ego_scene(), K.ego_stated()
    assert (rig.focal_px, rig.cx, rig.cy, rig.baseline_m) == (s["focal_px"], s["cx"], s["cy"], s["baseline_m"]) and np.array_equal(rig.Q, s["Q"])
    Rm, t = K.EGO_MOTION
    disp, status = s["disp"], s["status"]
    fits = []
    for d0, d1 in ((disp[0], disp[1]), (DeviceMat.from_host(vp.default_context(), disp[0]), DeviceMat.from_host(vp.default_context(), disp[1]))):
        fit = rig.ego_motion(d0, d1, s["prev"], s["next"], status, return_mask=True, **K.EGO_SEARCH)
        fits.append(fit)
        _same(fit, want, "ego motion")
        assert np.array_equal(fit.mask, want["inliers"]) and not fit.mask[~status].any()
        ang, dt = K.rot_angle(fit.R, Rm), float(np.linalg.norm(fit.t - t))
        print("ego motion: angle %r rad (bound %r), |dt| %r m (bound %r), %d of %d" % (ang, K.EGO_BOUND_ROT, dt, K.EGO_BOUND_T, fit.n_inliers, fit.n_usable))
        assert ang <= K.EGO_BOUND_ROT and dt <= K.EGO_BOUND_T
        assert np.abs(fit.inverse().matrix @ fit.matrix - np.eye(4)).max() <= 1e-12
    assert np.array_equal(R.bits(fits[0].hypothesis), R.bits(fits[1].hypothesis)) and np.array_equal(fits[0].mask, fits[1].mask)
    # in metres with a threshold of 5 cm every pair of this scene is an inlier too, so the refit is the same least squares
    metric = rig.ego_motion(disp[0], disp[1], s["prev"], s["next"], status, space="metric", threshold=0.05, **K.EGO_SEARCH)
    assert metric.found and metric.n_inliers == fits[0].n_inliers == fits[0].n_usable
    assert K.rot_angle(metric.R, Rm) <= K.EGO_BOUND_ROT and float(np.linalg.norm(metric.t - t)) <= K.EGO_BOUND_T

