"""CPU suite for the calibration-time geometry (vision.utils.stereo.stereo_rectify, float64 numpy, no native library): properties every
rectification has, on three synthetic rigs.  The tolerances are what a few dozen double operations on values of order 10^3 leave
(1e-9 px, 1e-9 relative; 1e-12 for the rotations): a case that needs more is a wrong case."""
import numpy as np
import pytest

import rectify_restate as RR

SIZE = (640, 480)
WIDE = [-0.2853, 0.0912, 0.00053, -0.00031, -0.0137]                      # k1 k2 p1 p2 k3 of a wide lens


def _rot(rx, ry, rz):
    from vision.utils.stereo import rodrigues
    return rodrigues([0, 0, np.deg2rad(rz)]) @ rodrigues([0, np.deg2rad(ry), 0]) @ rodrigues([np.deg2rad(rx), 0, 0])


def _rig(name):
    K1 = np.array([[412.3, 0, 318.4], [0, 411.1, 243.9], [0, 0, 1.0]])
    K2 = np.array([[409.8, 0, 322.7], [0, 410.4, 238.2], [0, 0, 1.0]])
    if name == "horizontal":
        return K1, WIDE, K2, [-0.2791, 0.0875, -0.0004, 0.0006, -0.0121], _rot(1.0, -2.0, 3.0), np.array([-0.12, 0.004, -0.003])
    if name == "vertical":
        return K1, WIDE, K2, WIDE, _rot(-1.5, 1.0, 2.0), np.array([0.005, -0.12, 0.002])
    K = np.array([[500.0, 0, 310.5], [0, 500.0, 236.25], [0, 0, 1.0]])
    return K, None, K, None, np.eye(3), np.array([-0.1, 0.0, 0.0])


def _points(R, T, n=200):
    """points in the first camera's frame, in front of both cameras and inside both fields of view"""
    rng = np.random.default_rng(11)
    X = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.35, 0.35, n), rng.uniform(1.0, 6.0, n)], axis=-1)
    X[:, :2] *= X[:, 2:3]
    assert (X[:, 2] > 0).all() and ((R @ X.T).T + T)[:, 2].min() > 0
    return X


@pytest.fixture(scope="module", params=["horizontal", "vertical", "identity"])
def rig(request):
    from vision.utils import stereo
    K1, d1, K2, d2, R, T = _rig(request.param)
    out = stereo.stereo_rectify(K1, d1, K2, d2, SIZE, R, T)
    return dict(name=request.param, K1=K1, d1=d1, K2=K2, d2=d2, R=R, T=T, out=out, axis=1 if request.param == "vertical" else 0)


def test_rodrigues_round_trip():
    from vision.utils.stereo import rodrigues
    rng = np.random.default_rng(3)
    for v in [rng.normal(size=3) * s for s in (1e-9, 1e-3, 0.5, 2.0)] + [np.array([np.pi - 1e-7, 0, 0]), np.array([0, 0, np.pi]), np.zeros(3)]:
        M = rodrigues(v)
        assert np.abs(M.T @ M - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(M) - 1) < 1e-12
        back = rodrigues(M)
        assert np.abs(rodrigues(back) - M).max() < 1e-9
        if np.linalg.norm(v) < np.pi - 1e-3:
            assert np.abs(back - v).max() < 1e-9
    assert np.allclose(rodrigues([0, 0, np.pi / 2]), [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)


def test_rotations_are_rotations(rig):
    R1, R2 = rig["out"][:2]
    for M in (R1, R2):
        assert np.abs(M.T @ M - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(M) - 1) < 1e-12
    assert np.abs(R2.T @ R1 - rig["R"]).max() < 1e-12, "the two rectifying rotations differ by the rig's rotation: R1 = R2 R"


def test_epipolar_lines_disparity_and_q(rig):
    """P2 carries the baseline in its fourth column, for points given in the rectified FIRST camera's frame: the second camera's pixel
    of X is P2 [R1 X; 1], and it is also what the rectified second camera sees of its own point R2 (R X + T) through P2's 3x3 part.
    (Applying the whole of P2 to R2 (R X + T) would count the baseline twice.)"""
    R1, R2, P1, P2, Q = rig["out"][:5]
    X = _points(rig["R"], rig["T"])
    a, across = rig["axis"], 1 - rig["axis"]
    Xr = (R1 @ X.T).T
    p1 = RR.project_rectified(Xr, P1)
    p2 = RR.project_rectified(Xr, P2)
    own = RR.project_rectified((R2 @ ((rig["R"] @ X.T).T + rig["T"]).T).T, np.concatenate([P2[:, :3], np.zeros((3, 1))], axis=1))
    assert np.abs(own - p2).max() < 1e-9, "P2's fourth column is the rotated baseline times the focal length"
    assert np.abs(p1[:, across] - p2[:, across]).max() < 1e-9, "corresponding points share their row (column for a vertical rig)"
    d = p1[:, a] - p2[:, a]
    want = P1[0, 0] * np.linalg.norm(rig["T"]) / Xr[:, 2]
    assert np.abs(d / want - 1).max() < 1e-9
    if a == 0:
        back = (Q @ np.stack([p1[:, 0], p1[:, 1], d, np.ones(len(d))], axis=0)).T
        back = back[:, :3] / back[:, 3:4]
        assert np.abs(back / Xr - 1).max() < 1e-9, "Q takes (x, y, d, 1) back to the point in the rectified first camera"


def test_maps_invert_the_raw_camera_model(rig):
    """a point seen through the raw camera (with distortion) lies where the rectification map of its rounded rectified pixel points,
    to within the map's local gradient times the half pixel of the rounding"""
    from vision.utils.transform import _undistort_coords
    R1, R2, P1, P2 = rig["out"][:4]
    X = _points(rig["R"], rig["T"])
    for K, d, Rk, Pk, Xc in ((rig["K1"], rig["d1"], R1, P1, X), (rig["K2"], rig["d2"], R2, P2, (rig["R"] @ X.T).T + rig["T"])):
        u, v = _undistort_coords("test", K, d, Rk, Pk, SIZE)
        raw = RR.project_raw(Xc, K, d)
        p = RR.project_rectified((Rk @ Xc.T).T, np.concatenate([Pk[:, :3], np.zeros((3, 1))], axis=1))
        xi, yi = np.rint(p[:, 0]).astype(int), np.rint(p[:, 1]).astype(int)
        ok = (xi >= 1) & (xi < SIZE[0] - 1) & (yi >= 1) & (yi < SIZE[1] - 1)
        assert ok.sum() > 100
        xi, yi, raw = xi[ok], yi[ok], raw[ok]
        for m, col in ((u, 0), (v, 1)):
            gx = np.maximum(np.abs(m[yi, xi + 1] - m[yi, xi]), np.abs(m[yi, xi] - m[yi, xi - 1]))
            gy = np.maximum(np.abs(m[yi + 1, xi] - m[yi, xi]), np.abs(m[yi, xi] - m[yi - 1, xi]))
            bound = 0.5 * (gx + gy) * 1.05 + 1e-9                  # first order, with 5 % for the map's curvature over half a pixel
            assert (np.abs(m[yi, xi] - raw[:, col]) <= bound).all()


def _taps_inside(K, d, Rk, Pk, roi):
    from vision.utils.transform import _fixed_from_double, _undistort_coords
    u, v = _undistort_coords("test", K, d, Rk, Pk, SIZE)
    xy, _ = _fixed_from_double(u, v)
    x, y, w, h = roi
    sx, sy = xy[y:y + h, x:x + w, 0].astype(int), xy[y:y + h, x:x + w, 1].astype(int)
    return bool(((sx >= 0) & (sx + 1 <= SIZE[0] - 1) & (sy >= 0) & (sy + 1 <= SIZE[1] - 1)).all())


@pytest.mark.parametrize("name", ["horizontal", "vertical"])
def test_alpha_zero_leaves_no_invalid_pixel_in_the_rois(name):
    from vision.utils import stereo
    K1, d1, K2, d2, R, T = _rig(name)
    R1, R2, P1, P2, Q, roi1, roi2 = stereo.stereo_rectify(K1, d1, K2, d2, SIZE, R, T, alpha=0)
    for K, d, Rk, Pk, roi in ((K1, d1, R1, P1, roi1), (K2, d2, R2, P2, roi2)):
        assert roi[2] > SIZE[0] // 2 and roi[3] > SIZE[1] // 2, "the valid rectangle is most of the image"
        assert 0 <= roi[0] and roi[0] + roi[2] <= SIZE[0] and 0 <= roi[1] and roi[1] + roi[3] <= SIZE[1]
        assert _taps_inside(K, d, Rk, Pk, roi), "a pixel of the valid rectangle has a tap outside the source"
    assert max(SIZE[0] - roi1[2], SIZE[0] - roi2[2]) <= 2 and max(SIZE[1] - roi1[3], SIZE[1] - roi2[3]) <= 2, "alpha = 0: the inner rectangle fills the image"


@pytest.mark.parametrize("name", ["horizontal", "vertical"])
def test_alpha_one_keeps_every_source_border_pixel(name):
    from vision.utils import stereo
    from vision.utils.transform import _camera
    K1, d1, K2, d2, R, T = _rig(name)
    R1, R2, P1, P2 = stereo.stereo_rectify(K1, d1, K2, d2, SIZE, R, T, alpha=1)[:4]
    g = np.arange(9)
    gx, gy = np.meshgrid(g * (SIZE[0] - 1) / 8, g * (SIZE[1] - 1) / 8)
    border = (gx == 0) | (gy == 0) | (gx == SIZE[0] - 1) | (gy == SIZE[1] - 1)
    pts = np.stack([gx[border], gy[border]], axis=-1)
    for K, d, Rk, Pk in ((K1, d1, R1, P1), (K2, d2, R2, P2)):
        p = stereo._undistort_points(pts, *_camera("test", K, d), Rk, Pk)
        rays = (Rk.T @ np.linalg.inv(Pk[:, :3]) @ np.concatenate([p, np.ones((len(p), 1))], axis=1).T).T
        assert np.abs(RR.project_raw(rays, K, d) - pts).max() < 1e-6, "the fixed-point inversion of the distortion has converged on the border of a wide lens"
        assert p[:, 0].min() >= -1e-9 and p[:, 0].max() <= SIZE[0] - 1 + 1e-9 and p[:, 1].min() >= -1e-9 and p[:, 1].max() <= SIZE[1] - 1 + 1e-9


def test_identity_rig():
    from vision.utils import stereo
    K, d, _, _, R, T = _rig("identity")
    R1, R2, P1, P2, Q, roi1, roi2 = stereo.stereo_rectify(K, d, K, d, SIZE, R, T)
    assert np.array_equal(R1, np.eye(3)) and np.array_equal(R2, np.eye(3))
    assert np.abs(P1[:, :3] - K).max() < 1e-9 and not P1[:, 3].any()
    assert np.abs(P2[:, :3] - K).max() < 1e-9 and abs(P2[0, 3] - P1[0, 0] * T[0]) < 1e-9 and P2[1, 3] == 0 and P2[2, 3] == 0
    assert np.abs(Q - stereo.reprojection_matrix(P1[0, 0], P1[0, 2], P1[1, 2], 0.1)).max() < 1e-9
    assert np.abs(stereo.reprojection_matrix(500, 310.5, 236.25, 0.1, cx_right=300.5) - [[1, 0, 0, -310.5], [0, 1, 0, -236.25], [0, 0, 0, 500], [0, 0, 10, -100]]).max() < 1e-12
    assert roi1 == roi2 == (0, 0, SIZE[0] - 1, SIZE[1] - 1), "the last column and row have a tap (of weight 0) outside"
    # scaled to another size with alpha = 0 the identity stays a pure scale
    P1s = stereo.stereo_rectify(K, d, K, d, SIZE, R, T, alpha=0, new_size=(320, 240))[2]
    assert abs(P1s[0, 0] / 500 - 319 / 639) < 1e-3 and abs(P1s[0, 2] - 310.5 * 319 / 639) < 1e-9


def test_refusals():
    from vision.utils import stereo
    from vision.utils.helpers import error
    K, d, _, _, R, T = _rig("identity")
    ok = lambda **o: stereo.stereo_rectify(*[o.get(k, v) for k, v in (("K1", K), ("d1", d), ("K2", K), ("d2", d), ("size", SIZE), ("R", R), ("T", T))],
                                           **{k: v for k, v in o.items() if k in ("alpha", "new_size", "zero_disparity")})
    ok()
    skew = np.eye(3)
    skew[0, 1] = 1e-5
    bad = [dict(R=np.full((3, 3), np.nan)), dict(R=skew), dict(R=2 * np.eye(3)), dict(R=np.eye(4)), dict(T=[0, 0, 0]), dict(T=[np.inf, 0, 0]), dict(T=[1, 2]),
           dict(alpha=-0.5), dict(alpha=1.01), dict(alpha=float("nan")), dict(size=(0, 480)), dict(size=(640, -1)), dict(new_size=(0, 0)), dict(new_size=(320, 0)),
           dict(d1=[0.1] * 9 + [0.01, 0, 0]), dict(d2=[0.1] * 8 + [0] * 4 + [0.01, 0]), dict(d1=[0.1] * 3), dict(K1=np.eye(4)), dict(K2=np.full((3, 3), np.inf))]
    for o in bad:
        with pytest.raises((error, ValueError)):
            ok(**o)
    for args in ((0, 300, 200, 0.1), (500, 300, 200, 0), (500, np.nan, 200, 0.1), (500, 300, 200, -0.1)):
        with pytest.raises(ValueError):
            stereo.reprojection_matrix(*args)
    with pytest.raises(ValueError):
        stereo.StereoRig(*_rig("vertical")[:4], SIZE, *_rig("vertical")[4:])
