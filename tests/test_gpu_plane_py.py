"""GPU suite of the Python layer of plane fitting (vision.utils.stereo.fit_plane, fit_planes, StereoRig.fit_plane; DESIGN.md section
4.38) against the statement tests/plane_restate.py and against analytic disparity planes."""
import numpy as np
import pytest

import plane_cases as K
import plane_restate as R

pytestmark = pytest.mark.gpu
W, H = 96, 64
DISPARITY_PLANES = [(0.05, 0.02, 12.0), (-0.08, 0.03, 20.0), (0.0, -0.1, 18.0)]


def _same(fit, want, what):
    assert fit.found == want["found"] and (fit.usable, fit.inliers, fit.hypotheses) == (want["n_usable"], want["n_inliers"], want["n_hypotheses"]), what
    assert np.array_equal(R.bits(fit.hypothesis), R.bits(want["result"][4:8])), what
    got = {"result": np.concatenate([fit.normal, [fit.d], fit.hypothesis, fit.centroid, [fit.rms]])}
    K.same_refit(got, want, what)


def test_numpy_in_numpy_out_device_in_device_out(vp):
    from vision.devmat import DeviceMat
    from vision.utils import stereo
    for cid in ("box_and_mask_and_holes", "two_planes_60_40", "two_points"):
        c, want = K.BY_ID[cid], K.stated(cid)
        kw = dict(box=c.box, threshold=c.threshold, max_iters=c.max_iters, confidence=c.confidence, seed=c.seed, along_z=c.metric == R.ALONG_Z)
        a = stereo.fit_plane(c.xyz, mask=c.mask, return_mask=True, **kw)
        assert isinstance(a.mask, np.ndarray) and np.array_equal(a.mask, want["inliers"])
        _same(a, want, cid)
        assert stereo.fit_plane(c.xyz, mask=c.mask, **kw).mask is None
        ctx = vp.default_context()
        dm = None if c.mask is None else DeviceMat.from_host(ctx, c.mask)
        b = stereo.fit_plane(DeviceMat.from_host(ctx, c.xyz), mask=dm, return_mask=True, **kw)
        assert isinstance(b.mask, DeviceMat) and np.array_equal(b.mask.host(), want["inliers"])
        _same(b, want, cid + " device")
        if c.mask is not None:                                   # numpy points with a device mask: a host mask back
            m = stereo.fit_plane(c.xyz, mask=dm, return_mask=True, **kw)
            assert isinstance(m.mask, np.ndarray) and np.array_equal(m.mask, want["inliers"])


def test_point_list_equals_the_image_of_the_same_points(vp):
    from vision.utils import stereo
    c = K.BY_ID["two_planes_60_40"]
    want = K.stated(c.id)
    kw = dict(threshold=c.threshold, max_iters=c.max_iters, seed=c.seed)
    a = stereo.fit_plane(c.xyz.reshape(-1, 3), return_mask=True, **kw)
    _same(a, want, "list")
    assert a.mask.shape == (c.w * c.h,) and np.array_equal(a.mask, want["inliers"].reshape(-1))
    with pytest.raises(ValueError):
        stereo.fit_plane(c.xyz.reshape(-1, 3), box=(0, 0, 1, 1))


def test_fit_planes_peels_two_planes_and_stops(vp):
    from vision.devmat import DeviceMat
    from vision.utils import stereo
    xyz, label = K.scene(W, H, [K.P1, K.P2], [55, 30], K.SIGMA, 0.15, 77)
    kw = dict(threshold=4 * K.SIGMA, max_iters=512, seed=3)
    # the statement's peel
    cand, peel = np.full((H, W), 255, np.uint8), []
    for _ in range(3):
        w = R.fit(xyz, mask=cand, metric=R.PERP, confidence=0.99, **kw)
        if not w["found"] or w["n_inliers"] < 400:
            break
        peel.append(w)
        cand = cand & ~w["inliers"]
    assert len(peel) == 2 and peel[0]["n_inliers"] > peel[1]["n_inliers"] > 1000
    for points in (xyz, DeviceMat.from_host(vp.default_context(), xyz)):
        fits = stereo.fit_planes(points, 3, 400, **kw)
        assert len(fits) == 2
        masks = [np.asarray(f.mask.host() if isinstance(f.mask, DeviceMat) else f.mask) for f in fits]
        assert all(isinstance(f.mask, type(points)) for f in fits)
        assert not (masks[0] & masks[1]).any(), "the masks are disjoint"
        for f, m, w, truth in zip(fits, masks, peel, (K.P1, K.P2)):
            assert np.array_equal(m, w["inliers"])
            _same(f, w, "peel")
            t = K.plane_of(*truth)
            assert K.angle(f.normal, t[:3]) < 0.01 and abs(f.d - t[3]) < 0.01
        assert np.array_equal(masks[0] | masks[1], peel[0]["inliers"] | peel[1]["inliers"])
    assert stereo.fit_planes(xyz, 1, 400, **kw)[0].inliers == peel[0]["n_inliers"]
    assert stereo.fit_planes(xyz, 3, H * W, **kw) == []


@pytest.fixture(scope="module")
def rig(vp):
    from vision.utils import stereo
    K1 = np.array([[112.3, 0, 47.4], [0, 111.1, 31.9], [0, 0, 1.0]])
    K2 = np.array([[109.8, 0, 48.7], [0, 110.4, 30.2], [0, 0, 1.0]])
    return stereo.StereoRig(K1, [-0.28, 0.09, 0.0005, -0.0003, -0.013], K2, [-0.27, 0.08, -0.0004, 0.0006, -0.012], (W, H), stereo.rodrigues([0.01, -0.02, 0.03]),
                            [-0.12, 0.004, -0.003])


@pytest.mark.parametrize("abc", DISPARITY_PLANES, ids=["a", "b", "c"])
def test_rig_fits_an_analytic_disparity_plane(vp, rig, abc):
    from vision.devmat import DeviceMat
    from vision.utils import stereo
    a, b, c = abc
    r = np.random.default_rng(int(c))
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    exact = a * x + b * y + c
    disp = np.rint(exact * 16).astype(np.int16)
    invalid = stereo.invalid_disparity(0)
    gross = r.random((H, W)) < 0.10
    disp[gross] = r.integers(16, 60 * 16, int(gross.sum()))
    disp[20:26] = invalid
    good = ~gross
    good[20:26] = False
    kw = dict(threshold=0.25, max_iters=1000, seed=1)
    for d in (disp, DeviceMat.from_host(vp.default_context(), disp)):
        fit = rig.fit_plane(d, return_mask=True, **kw)
        assert fit.found and fit.usable == H * W - 6 * W
        mask = np.asarray(fit.mask.host() if isinstance(fit.mask, DeviceMat) else fit.mask)
        assert (mask[good] == 255).all(), "a valid pixel of the plane is not an inlier"
        # the refit plane, carried back to disparity space, against the analytic plane: within the rounding of a sixteenth
        pd = np.append(fit.normal, fit.d) @ rig.Q
        back = -(pd[0] * x + pd[1] * y + pd[3]) / pd[2]
        err = float(np.abs(back - exact).max())
        print("plane %s: largest difference %.5f px" % (abc, err))
        assert err <= 1 / 32
        # the metric plane is pi Q^-1 of the plane found in disparity space
        flat = stereo.fit_plane(stereo.reproject_to_3d(disp, np.eye(4), invalid), along_z=True, **kw)
        assert np.array_equal(R.bits(flat.hypothesis), R.bits(fit.hypothesis)), "the hypothesis stays in disparity space"
        pm = np.append(flat.normal, flat.d) @ np.linalg.inv(rig.Q)
        pm = pm / np.linalg.norm(pm[:3])
        pm = pm if pm[3] > 0 else -pm
        assert np.allclose(np.append(fit.normal, fit.d), pm, rtol=1e-12, atol=0) and fit.d > 0 and abs(np.linalg.norm(fit.normal) - 1) < 1e-12
        # the same surface in metres: the metric search agrees on where it is
        metric = rig.fit_plane(d, space="metric", threshold=0.05, max_iters=1000, seed=1)
        assert metric.found and K.angle(metric.normal, fit.normal) < 0.05
