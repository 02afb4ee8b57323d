"""CPU suite for the statement of cv2.remap / convertMaps / warpPerspective (tests/remap_restate.py): the
restatement is checked against things it was not written from - identities, integer shifts, the warpAffine oracle on maps both
arithmetics compute exactly, its own two map forms, cvRound's ties and the int16 saturation - and the facade's host functions
(initUndistortRectifyMap, getPerspectiveTransform, perspectiveTransform) against an extended-precision evaluation and known answers."""
import numpy as np
import pytest

import remap_restate as R


def _img(h, w, cn, seed=0):
    rng = np.random.default_rng(1000 * h + 10 * w + cn + seed)
    return rng.integers(0, 256, (h, w) if cn == 1 else (h, w, cn), dtype=np.uint8)


def _grid(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return x.astype(np.float32), y.astype(np.float32)


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_identity_maps_give_the_source_back(cn):
    img = _img(23, 31, cn)
    mx, my = _grid(23, 31)
    for nearest in (False, True):
        for border in ("constant", "replicate"):
            assert np.array_equal(R.remap_restate(img, mx, my, nearest, border, (9, 8, 7, 6)), img)
    assert np.array_equal(R.remap_restate(img, np.dstack([mx, my])), img)
    assert np.array_equal(R.warp_perspective_restate(img, np.eye(3), (31, 23)), img)
    assert np.array_equal(R.warp_perspective_restate(img, np.eye(3), (31, 23), inverse_map=True, nearest=True), img)


def test_integer_shifts_give_the_shifted_image_with_the_border():
    img = _img(20, 30, 3)
    mx, my = _grid(20, 30)
    val = (11, 22, 33)
    for nearest in (False, True):
        out = R.remap_restate(img, mx + 7, my - 3, nearest, "constant", val)
        exp = np.empty_like(img)
        exp[:] = val
        exp[3:, :23] = img[:17, 7:]
        assert np.array_equal(out, exp)
        rep = R.remap_restate(img, mx + 7, my - 3, nearest, "replicate")
        assert np.array_equal(rep, img[np.clip(np.arange(20) - 3, 0, 19)][:, np.clip(np.arange(30) + 7, 0, 29)])
    # every tap outside: the border value itself, or the nearest edge pixel
    assert (R.remap_restate(img, mx + 100, my, False, "constant", val) == np.array(val)).all()
    assert np.array_equal(R.remap_restate(img, mx + 100, my, False, "replicate"), np.repeat(img[:, -1:], 30, axis=1))


AFFINE = [np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), np.array([[0.75, 0.25, -3.5], [-0.125, 1.25, 2.96875]]),
          np.array([[1.03125, -0.5, 10.0], [0.5, 0.90625, -7.03125]]), np.array([[-1.0, 0.0, 40.15625], [0.0, -0.5, 30.0]])]


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("border", ["constant", "replicate"])
def test_affine_maps_equal_the_warp_affine_oracle(oracle, cn, border):
    """matrix entries and offsets are multiples of 1/32 and coordinates stay under 1024: float32 maps, warpAffine's 22.10 fixed
    point and warpPerspective's doubles are all exact, so all three must sample identically"""
    img = _img(41, 57, cn)
    dw, dh = 61, 45
    x, y = _grid(dh, dw)
    val = (200, 100, 50)[:cn] if cn > 1 else 77
    for M in AFFINE:
        assert np.array_equal(M * 32, np.rint(M * 32))
        mx = (np.float32(M[0, 0]) * x + np.float32(M[0, 1]) * y + np.float32(M[0, 2])).astype(np.float32)
        my = (np.float32(M[1, 0]) * x + np.float32(M[1, 1]) * y + np.float32(M[1, 2])).astype(np.float32)
        exp = oracle.warp_affine(img, M, (dw, dh), inverse_map=True, border=border, value=val)
        assert np.array_equal(R.remap_restate(img, mx, my, False, border, val), exp)
        H = np.vstack([M, [0.0, 0.0, 1.0]])
        assert np.array_equal(R.warp_perspective_restate(img, H, (dw, dh), inverse_map=True, border=border, value=val), exp)


def test_forward_homography_with_an_affine_last_row_equals_the_oracle(oracle):
    img = _img(33, 47, 3)
    M = np.array([[0.5, 0.0, 3.0], [0.0, 2.0, -4.0]])          # inverse: entries 2, 0.5, offsets -6, 2: exact in both
    H = np.vstack([M, [0.0, 0.0, 1.0]])
    for border in ("constant", "replicate"):
        exp = oracle.warp_affine(img, M, (50, 40), border=border, value=(1, 2, 3))
        assert np.array_equal(R.warp_perspective_restate(img, H, (50, 40), border=border, value=(1, 2, 3)), exp)
    assert np.array_equal(R.invert33_restate(H), [[2.0, 0.0, -6.0], [0.0, 0.5, 2.0], [0.0, 0.0, 1.0]])
    assert np.array_equal(R.invert33_restate(np.ones((3, 3))), np.zeros((3, 3)))


def test_the_fixed_form_and_the_float_form_agree():
    rng = np.random.default_rng(5)
    img = _img(37, 29, 3)
    mx = (rng.integers(-3 * 64, (29 + 3) * 64, (40, 50)) / 64).astype(np.float32)
    my = (rng.integers(-3 * 64, (37 + 3) * 64, (40, 50)) / 64).astype(np.float32)
    for nearest in (False, True):
        xy, frac = R.convert_maps_restate(mx, my, nearest)
        assert xy.dtype == np.int16 and (frac is None) == nearest
        for border in ("constant", "replicate"):
            a = R.remap_restate(img, mx, my, nearest, border, (5, 6, 7))
            assert np.array_equal(R.remap_restate(img, xy, frac, nearest, border, (5, 6, 7)), a)
            assert np.array_equal(R.remap_restate(img, np.dstack([mx, my]), None, nearest, border, (5, 6, 7)), a)
    xy, frac = R.convert_maps_restate(mx, my)
    assert np.array_equal(R.remap_restate(img, xy, frac | 0xfc00), R.remap_restate(img, xy, frac)), "only ten bits of the fraction plane count"


def test_ties_round_to_even_and_large_coordinates_saturate():
    k = np.arange(-9, 10, dtype=np.float32)
    mx = (k / 64)[None, :]                                    # mx * 32 = k / 2: every odd k is a tie
    xy, frac = R.convert_maps_restate(mx, np.zeros_like(mx))
    ix = np.array([-4, -4, -4, -3, -2, -2, -2, -1, 0, 0, 0, 1, 2, 2, 2, 3, 4, 4, 4])
    assert np.array_equal(xy[0, :, 0], ix >> 5) and np.array_equal(frac[0], ix & 31)
    n = np.float32([[-2.5, -1.5, -0.5, 0.5, 1.5, 2.5]])
    assert np.array_equal(R.convert_maps_restate(n, n, nearest=True)[0][0, :, 0], [-2, -2, 0, 0, 2, 2])
    big = np.float32([[32767.0, 32768.0, 40000.0, 6.0e7, -32768.0, -32769.0, -6.0e7, 32767.96875]])
    xy, frac = R.convert_maps_restate(big, big)
    assert np.array_equal(xy[0, :, 0], [32767, 32767, 32767, 32767, -32768, -32768, -32768, 32767])
    assert frac[0, 7] == 31 * 32 + 31
    assert np.array_equal(R.convert_maps_restate(big, big, nearest=True)[0][0, :, 1], [32767, 32767, 32767, 32767, -32768, -32768, -32768, 32767])
    img = _img(5, 7, 1)
    assert (R.remap_restate(img, big, big, False, "constant", 9) == 9).all()
    assert np.array_equal(R.remap_restate(img, big, big, True, "replicate")[0], [img[4, 6]] * 4 + [img[0, 0]] * 3 + [img[4, 6]])
    # warpPerspective: a scale that sends coordinates past int32 clamps before the rounding
    sx, sy, frac = R.warp_perspective_coords(np.diag([1e9, -1e9, 1.0]), (4, 3), inverse_map=True)
    assert sx[1, 1] == 32767 and sy[1, 1] == -32768 and sx[0, 0] == 0


def test_block_origin_and_zero_denominator():
    assert [R.block_width(w, h) for w, h in ((63, 3), (64, 15), (65, 16), (129, 17), (2000, 1), (400, 3))] == [63, 64, 64, 64, 1024, 341]
    # W = 0 exactly at x = 8 of row 0: that pixel maps to (0, 0)
    M = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.125, 0.0, -1.0]])
    sx, sy, frac = R.warp_perspective_coords(M, (16, 2), inverse_map=True)
    assert (sx[0, 8], sy[0, 8], frac[0, 8]) == (0, 0, 0)
    assert sx[0, 7] == -56 and sx[0, 9] == 72


# ---- the facade's host functions ----------------------------------------------------------------------------------------------------

K = np.array([[812.5, 0.0, 318.25], [0.0, 809.75, 243.5], [0.0, 0.0, 1.0]])
NEWK = np.array([[700.0, 0.0, 320.0], [0.0, 700.0, 240.0], [0.0, 0.0, 1.0]])
DIST = {4: [-0.31, 0.12, 0.0011, -0.0007], 5: [-0.31, 0.12, 0.0011, -0.0007, -0.02], 8: [-0.31, 0.12, 0.0011, -0.0007, -0.02, 0.01, -0.003, 0.0005]}


def _model_longdouble(Kc, dist, Rm, Kn, size):
    L = np.longdouble
    w, h = size
    k = np.zeros(8, L)
    k[:len(dist)] = np.asarray(dist, L)
    ir = np.linalg.inv(np.asarray(Kn, np.float64) @ np.asarray(Rm, np.float64)).astype(L)
    j, i = np.meshgrid(np.arange(w).astype(L), np.arange(h).astype(L))
    X, Y, W = (ir[r, 0] * j + ir[r, 1] * i + ir[r, 2] for r in range(3))
    x, y = X / W, Y / W
    r2 = x * x + y * y
    kr = (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2) / (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2)
    xd = x * kr + k[2] * 2 * x * y + k[3] * (r2 + 2 * x * x)
    yd = y * kr + k[2] * (r2 + 2 * y * y) + k[3] * 2 * x * y
    return L(Kc[0, 0]) * xd + L(Kc[0, 2]), L(Kc[1, 1]) * yd + L(Kc[1, 2])


def _within_one_ulp(got, exact):
    assert got.dtype == np.float32
    ulp = np.spacing(np.maximum(np.abs(got), np.abs(exact.astype(np.float32)))).astype(np.longdouble)
    return bool((np.abs(got.astype(np.longdouble) - exact) <= ulp).all())


@pytest.mark.parametrize("ncoef", [4, 5, 8])
def test_init_undistort_rectify_map_follows_the_distortion_model(ncoef):
    from vision import cv2_facade as f
    a = 0.02
    Rm = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    size = (160, 120)
    for Rmat in (None, Rm):
        eu, ev = _model_longdouble(K, DIST[ncoef], np.eye(3) if Rmat is None else Rmat, NEWK, size)
        mx, my = f.initUndistortRectifyMap(K, DIST[ncoef], Rmat, NEWK, size, f.CV_32FC1)
        assert mx.shape == my.shape == (120, 160)
        assert _within_one_ulp(mx, eu) and _within_one_ulp(my, ev)
        m2, empty = f.initUndistortRectifyMap(K, DIST[ncoef], Rmat, NEWK, size, f.CV_32FC2)
        assert m2.shape == (120, 160, 2) and empty.size == 0 and np.array_equal(m2[:, :, 0], mx) and np.array_equal(m2[:, :, 1], my)
        xy, frac = f.initUndistortRectifyMap(K, DIST[ncoef], Rmat, NEWK, size, f.CV_16SC2)
        assert xy.dtype == np.int16 and xy.shape == (120, 160, 2) and frac.dtype == np.uint16 and frac.shape == (120, 160)
        back = xy[:, :, 0].astype(np.float64) + (frac & 31) / 32.0
        assert np.abs(back - eu.astype(np.float64)).max() <= 1 / 64 + 1e-9


def test_zero_distortion_with_the_same_camera_matrix_is_the_identity_grid():
    """The bound is one float32 ulp at the coordinate's magnitude, which at coordinate 0 admits no error at all.  With focal lengths
    that are powers of two and a principal point on a binary grid every operation of the model is exact in float64, so the grid must
    come back exactly.  For a general camera matrix (fx (j - cx) / fx + cx) the float64 evaluation itself carries a few ulps of
    float64 at the principal point's magnitude (about 1e-13 here): there the ulp is taken at max(|coordinate|, |principal point|)."""
    from vision import cv2_facade as f
    gx, gy = _grid(70, 90)
    KE = np.array([[512.0, 0.0, 44.25], [0.0, 1024.0, 35.5], [0.0, 0.0, 1.0]])
    for dist in (None, [0, 0, 0, 0], np.zeros(14)):
        mx, my = f.initUndistortRectifyMap(KE, dist, None, KE, (90, 70), f.CV_32FC1)
        assert _within_one_ulp(mx, gx.astype(np.longdouble)) and _within_one_ulp(my, gy.astype(np.longdouble))
        mx, my = f.initUndistortRectifyMap(K, dist, None, K, (90, 70), f.CV_32FC1)
        assert (np.abs(mx - gx) <= np.spacing(np.maximum(gx, np.float32(K[0, 2])))).all()
        assert (np.abs(my - gy) <= np.spacing(np.maximum(gy, np.float32(K[1, 2])))).all()


def test_get_perspective_transform_maps_its_points_and_perspective_transform_known_answers():
    from vision import cv2_facade as f
    src = np.float32([[10, 20], [300, 15], [310, 220], [5, 230]])
    dst = np.float32([[0, 0], [200, 0], [200, 150], [0, 150]])
    M = f.getPerspectiveTransform(src, dst)
    assert M.shape == (3, 3) and M.dtype == np.float64 and M[2, 2] == 1.0
    p = np.hstack([src.astype(np.float64), np.ones((4, 1))]) @ M.T
    p = p[:, :2] / p[:, 2:]
    assert np.abs(p - dst).max() <= 1e-9 * max(np.abs(dst).max(), 1.0)
    for shape in ((4, 1, 2), (4, 2)):
        q = f.perspectiveTransform(src.reshape(shape), M)
        assert q.shape == shape and q.dtype == np.float32 and np.abs(q.reshape(4, 2) - dst).max() <= 1e-3
    T = np.array([[2.0, 0.0, 1.0], [0.0, 3.0, -1.0], [0.0, 0.0, 2.0]])
    assert np.array_equal(f.perspectiveTransform(np.float64([[[1, 1]], [[0, 0]], [[-2, 4]]]), T), np.float64([[[1.5, 1.0]], [[0.5, -0.5]], [[-1.5, 5.5]]]))
    Z = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 0.0, -1.0]])       # w = 0 at x = 1: cv2 writes 0
    assert np.array_equal(f.perspectiveTransform(np.float64([[[1, 5]], [[2, 4]]]), Z), np.float64([[[0, 0]], [[2, 4]]]))
    assert np.allclose(f.getPerspectiveTransform(src, src), np.eye(3), atol=1e-9)


def test_facade_rejects_what_is_outside_the_path_before_anything_runs():
    from vision import cv2_facade as f
    from vision.utils import transform
    g = np.zeros((6, 5), np.uint8)
    mx, my = _grid(6, 5)
    xy = np.zeros((6, 5, 2), np.int16)
    fr = np.zeros((6, 5), np.uint16)
    bad = [lambda: f.remap(g, mx, my, 2), lambda: f.remap(g, mx, my, f.INTER_LINEAR, None, f.BORDER_REFLECT_101), lambda: f.remap(g, mx, my, f.INTER_LINEAR, None, f.BORDER_WRAP),
           lambda: f.remap(g.astype(np.float32), mx, my, f.INTER_LINEAR), lambda: f.remap(g.astype(np.uint16), mx, my, f.INTER_LINEAR),
           lambda: f.remap(np.zeros((6, 5, 5), np.uint8), mx, my, f.INTER_LINEAR), lambda: f.remap(np.zeros((0, 5), np.uint8), mx, my, f.INTER_LINEAR),
           lambda: f.remap(g, mx, my[:5], f.INTER_LINEAR), lambda: f.remap(g, mx.astype(np.float64), my.astype(np.float64), f.INTER_LINEAR),
           lambda: f.remap(g, mx, None, f.INTER_LINEAR), lambda: f.remap(g, xy, fr, f.INTER_NEAREST), lambda: f.remap(g, xy, None, f.INTER_LINEAR),
           lambda: f.remap(g, xy, fr.astype(np.float32), f.INTER_LINEAR), lambda: f.remap(g, fr, xy, f.INTER_LINEAR),
           lambda: f.remap(np.zeros((2, 32768), np.uint8), mx, my, f.INTER_LINEAR),
           lambda: f.warpPerspective(g, np.eye(2), (5, 6)), lambda: f.warpPerspective(g, np.eye(3), (0, 6)), lambda: f.warpPerspective(g, np.eye(3), (5, 6), flags=2),
           lambda: f.warpPerspective(g, np.eye(3), (5, 6), borderMode=f.BORDER_REFLECT), lambda: f.warpPerspective(g.astype(np.int16), np.eye(3), (5, 6)),
           lambda: f.warpPerspective(g, np.full((3, 3), np.nan), (5, 6)), lambda: f.warpPerspective(g, np.eye(3), 5),
           lambda: f.convertMaps(mx, my, f.CV_32FC1), lambda: f.convertMaps(xy, fr, f.CV_16SC2), lambda: f.convertMaps(mx, my, f.CV_32FC2),
           lambda: f.initUndistortRectifyMap(K, [0.1] * 4 + [0.0] * 4 + [1e-3] + [0.0] * 3, None, K, (8, 8), f.CV_32FC1),
           lambda: f.initUndistortRectifyMap(K, [0.1] * 4 + [0.0] * 8 + [0.01, 0.0], None, K, (8, 8), f.CV_32FC1),
           lambda: f.initUndistortRectifyMap(K, [0.1] * 3, None, K, (8, 8), f.CV_32FC1), lambda: f.initUndistortRectifyMap(K, None, None, K, (8, 8), f.CV_16UC1),
           lambda: f.initUndistortRectifyMap(np.eye(2), None, None, K, (8, 8), f.CV_32FC1), lambda: f.initUndistortRectifyMap(K, None, None, K, (0, 8), f.CV_32FC1),
           lambda: f.undistort(g.astype(np.float32), K, None), lambda: f.undistort(g, K, [0.0] * 12 + [0.1, 0.1]),
           lambda: f.getPerspectiveTransform(np.zeros((3, 2)), np.zeros((3, 2))), lambda: f.getPerspectiveTransform(np.zeros((4, 2)), np.zeros((4, 2))),
           lambda: f.perspectiveTransform(np.zeros((4, 1, 3), np.float32), np.eye(3)), lambda: f.perspectiveTransform(np.zeros((4, 1, 2), np.int32), np.eye(3))]
    for i, call in enumerate(bad):
        with pytest.raises(f.error):
            call()
            pytest.fail(f"case {i} was accepted")
    assert (f.INTER_NEAREST, f.INTER_LINEAR, f.WARP_INVERSE_MAP, f.CV_16UC1, f.CV_32FC1, f.CV_16SC2, f.CV_32FC2) == (0, 1, 16, 2, 5, 11, 13)
    for call in (lambda: transform.remap(g, mx, None), lambda: transform.remap(g.astype(np.int8), mx, my), lambda: transform.RemapTable(xy, fr)):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: transform.warp_perspective(g, np.eye(3), 0, 4), lambda: transform.remap(g, xy, fr, nearest=True), lambda: transform.remap(g, mx, my, border=4)):
        with pytest.raises(ValueError):
            call()
