"""GPU suite for vision.utils.stereo.StereoRig: from a raw side-by-side frame to depth, normals and points, byte for byte the composition
of the pieces called one by one, for both matchers; the identity rig; and nothing of the chain leaves HBM."""
import numpy as np
import pytest

import rectify_restate as R
import stereo_cases as StC

pytestmark = pytest.mark.gpu

W, H = 96, 64
BM = dict(num_disparities=16, block_size=9, uniqueness_ratio=5)
SGM = dict(num_disparities=16, block_size=5, uniqueness_ratio=5)
SPECKLE = dict(speckle_window_size=20, speckle_range=2, max_jump_m=0.5)


def _raw_frame():
    """a side-by-side BGR frame with texture and a shift between the eyes"""
    left, right = StC.shifted_pair(H, W, 6, 7, noise=50)
    rng = np.random.default_rng(2)
    tint = lambda g: np.stack([g, np.roll(g, 1, axis=0), 255 - g], axis=-1) // 2 + rng.integers(0, 40, (H, W, 3)).astype(np.uint8)
    return np.ascontiguousarray(np.concatenate([tint(left), tint(right)], axis=1).astype(np.uint8))


@pytest.fixture(scope="module")
def rig(vp):
    from vision.utils import stereo
    K1 = np.array([[112.3, 0, 47.4], [0, 111.1, 31.9], [0, 0, 1.0]])
    K2 = np.array([[109.8, 0, 48.7], [0, 110.4, 30.2], [0, 0, 1.0]])
    return stereo.StereoRig(K1, [-0.28, 0.09, 0.0005, -0.0003, -0.013], K2, [-0.27, 0.08, -0.0004, 0.0006, -0.012], (W, H), stereo.rodrigues([0.01, -0.02, 0.03]),
                            [-0.12, 0.004, -0.003])


def _bits(a):
    a = a.host_copy() if hasattr(a, "host_copy") else np.ascontiguousarray(a)
    return a.dtype, a.shape, a.tobytes()


@pytest.mark.parametrize("matcher", ["bm", "sgm"])
def test_rig_is_the_composition_of_the_pieces(vp, rig, matcher):
    from vision.devmat import DeviceMat
    from vision.utils import stereo
    args = BM if matcher == "bm" else SGM
    frame = _raw_frame()
    dframe = DeviceMat.from_host(vp.default_context(), frame)
    # the pieces, one by one
    gl, gr = stereo.rectify_pair(np.ascontiguousarray(frame[:, :W]), np.ascontiguousarray(frame[:, W:]), *rig.tables)
    disp = (stereo.disparity if matcher == "bm" else stereo.disparity_sgm)(gl, gr, **args)
    assert (disp != stereo.invalid_disparity(0)).sum() > 50, "the pair must leave something to measure"
    depth = stereo.depth_from_disparity(disp, rig.focal_px, rig.baseline_m)
    planes = (stereo.stereo_planes if matcher == "bm" else stereo.stereo_planes_sgm)(gl, gr, rig.focal_px, rig.baseline_m, cx=rig.cx, cy=rig.cy, **SPECKLE, **args)
    points = stereo.reproject_to_3d(disp, rig.Q, stereo.invalid_disparity(0))
    assert R.same_bits(points, R.reproject(disp, rig.Q, -16))
    known = disp > 0
    assert np.allclose(points[known][:, 2], depth[known], rtol=1e-6), "Q's Z is the depth plane's"
    # the rig, on a device frame: DeviceMats all the way
    got = rig.disparity(dframe, matcher=matcher, **args)
    assert isinstance(got, DeviceMat) and _bits(got) == _bits(disp)
    assert _bits(rig.depth(dframe, matcher=matcher, **args)) == _bits(depth)
    gd, gn = rig.planes(dframe, matcher=matcher, **SPECKLE, **args)
    assert isinstance(gd, DeviceMat) and isinstance(gn, DeviceMat) and _bits(gd) == _bits(planes[0]) and _bits(gn) == _bits(planes[1])
    pts = rig.points(got)
    assert isinstance(pts, DeviceMat) and _bits(pts) == _bits(points)
    # numpy in, numpy out; two images instead of one frame
    host = rig.planes(frame, matcher=matcher, **SPECKLE, **args)
    assert isinstance(host[0], np.ndarray) and _bits(host[0]) == _bits(planes[0]) and _bits(host[1]) == _bits(planes[1])
    two = rig.depth(np.ascontiguousarray(frame[:, :W]), np.ascontiguousarray(frame[:, W:]), matcher=matcher, **args)
    assert isinstance(two, np.ndarray) and _bits(two) == _bits(depth)
    assert _bits(rig.points(disp)) == _bits(points)


def test_identity_rig_is_the_matcher_on_the_grey_halves(vp):
    from vision.utils import stereo
    from vision.utils.color import bgr_to_gray
    K = np.array([[110.0, 0, 47.5], [0, 110.0, 31.5], [0, 0, 1.0]])
    rig = stereo.StereoRig(K, None, K, None, (W, H), np.eye(3), [-0.1, 0, 0])
    assert np.array_equal(rig.R1, np.eye(3)) and abs(rig.focal_px - 110) < 1e-9 and abs(rig.baseline_m - 0.1) < 1e-12
    frame = _raw_frame()
    left, right = np.ascontiguousarray(frame[:, :W]), np.ascontiguousarray(frame[:, W:])
    want = stereo.disparity(bgr_to_gray(left)[0], bgr_to_gray(right)[0], **BM)
    got = rig.disparity(frame, **BM)
    assert isinstance(got, np.ndarray) and _bits(got) == _bits(want)
    with pytest.raises(ValueError):
        rig.disparity(frame, matcher="census")


def test_nothing_in_the_chain_leaves_hbm(vp, rig, monkeypatch):
    """every image the chain makes is a DeviceMat whose device copy is the valid one and that has no host copy: the state a download
    would change (DeviceMat.host / host_copy are the only ways out, and both are counted here)"""
    from vision import devmat
    from vision.devmat import DeviceMat
    made, downloads = [], []
    init = DeviceMat.__init__

    def tracking_init(self, *a, **k):
        init(self, *a, **k)
        made.append(self)
    monkeypatch.setattr(DeviceMat, "__init__", tracking_init)
    for name in ("host", "host_copy"):
        orig = getattr(DeviceMat, name)
        monkeypatch.setattr(DeviceMat, name, lambda self, *a, _o=orig, _n=name, **k: (downloads.append(_n), _o(self, *a, **k))[1])
    dframe = DeviceMat.from_host(vp.default_context(), _raw_frame())
    made.clear()
    for matcher, args in (("bm", BM), ("sgm", SGM)):
        depth, normal = rig.planes(dframe, matcher=matcher, **SPECKLE, **args)
        pts = rig.points(rig.disparity(dframe, matcher=matcher, **args))
        assert all(isinstance(m, DeviceMat) for m in (depth, normal, pts))
    assert len(made) >= 2 * (2 + 3 + 2 + 2), "grey pair, disparity, depth, normals; grey pair, disparity, points - per matcher"
    assert not downloads, f"the chain downloaded: {downloads}"
    assert all(m._dev_ok and m._host is None for m in made), "an intermediate has a host copy"
    assert devmat.lazy_enabled()
