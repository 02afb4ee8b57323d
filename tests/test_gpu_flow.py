"""GPU suite of pyramidal Lucas-Kanade tracking (vision.utils.feature.track_points, cv2_facade.calcOpticalFlowPyrLK; libvp vp_flow.hip):
every case is compared bit for bit - positions, status and err - with the numpy statement tests/flow_restate.py.  Images of 96 x 80
to 320 x 240 and at most a few hundred points: windows and levels at their limits, points on, at and beyond the frame, lost points,
every stopping rule, the flags, point counts round the wave size, a strided level 0, reused pyramids and the back check."""
import functools

import numpy as np
import pytest

import flow_restate as R

pytestmark = pytest.mark.gpu

SHIFT = (2.3, -1.6)


@functools.lru_cache(maxsize=None)
def frames(h=120, w=160, seed=1, shift=SHIFT):
    a, b = R.texture(h, w, seed), R.texture(h, w, seed, shift)
    a.flags.writeable = b.flags.writeable = False
    return a, b


def grid(h, w, step=12, margin=24, frac=(0.25, 0.5)):
    ys, xs = np.mgrid[margin:h - margin:step, margin:w - margin:step]
    return np.stack([xs.ravel() + frac[0], ys.ravel() + frac[1]], 1).astype(np.float32)


def check(got, want, what=""):
    gp, gs, ge = got
    wp, ws, we = want
    gp = np.asarray(gp).reshape(-1, 2)
    bad = [i for i in range(len(wp)) if gp[i].tobytes() != wp[i].tobytes() or bool(gs[i]) != bool(ws[i]) or ge[i].tobytes() != we[i].tobytes()]
    assert not bad, (what, len(bad), len(wp), [(i, gp[i].tolist(), wp[i].tolist(), int(gs[i]), int(ws[i]), float(ge[i]), float(we[i])) for i in bad[:4]])
    assert len(gp) == len(wp) == len(gs) == len(ge)


def both(vp, a, b, pts, next_pts=None, win=(21, 21), max_level=3, max_count=30, eps=0.01, min_eig=1e-4, min_eigenvals=False):
    from vision.utils import feature
    flags = (R.OPTFLOW_USE_INITIAL_FLOW if next_pts is not None else 0) | (R.OPTFLOW_LK_GET_MIN_EIGENVALS if min_eigenvals else 0)
    want = R.lk_restate(a, b, pts, next_pts, win, max_level, max_count, eps, flags, min_eig)
    got = feature.track_points(a, b, pts, next_pts, win, max_level, max_count, eps, min_eig, min_eigenvals)
    assert got[0].shape == (len(want[0]), 1, 2) and got[0].dtype == np.float32 and got[1].dtype == bool and got[2].dtype == np.float32
    return got, want


def test_identical_frames_stay_where_they_are(vp):
    a, _ = frames()
    pts = grid(120, 160)
    got, want = both(vp, a, a, pts)
    check(got, want)
    assert got[0].reshape(-1, 2).tobytes() == pts.tobytes() and got[1].all() and not got[2].any()


@pytest.mark.parametrize("max_level", [0, 1, 3])
def test_shifted_texture(vp, max_level):
    a, b = frames()
    pts = grid(120, 160)
    got, want = both(vp, a, b, pts, max_level=max_level)
    check(got, want)
    assert got[1].all() and np.abs(got[0].reshape(-1, 2) - pts - np.float32(SHIFT)).max() < 0.1


def test_max_level_beyond_what_the_image_allows_is_the_clipped_call(vp):
    from vision.utils import feature
    a, b = frames(90, 100, 2)
    pts = grid(90, 100)
    got, want = both(vp, a, b, pts, max_level=15)
    check(got, want)
    assert feature.flow_level_count(100, 90, (21, 21), 15) == 3
    check(feature.track_points(a, b, pts, max_level=2), want)


@pytest.mark.parametrize("win,shape", [((3, 3), (96, 128)), ((4, 6), (96, 128)), ((5, 9), (96, 128)), ((21, 21), (96, 128)), ((31, 15), (96, 128)),
                                       ((63, 63), (144, 160))])
def test_windows(vp, win, shape):
    from vision.utils import feature
    a, b = frames(shape[0], shape[1], 3, (1.2, 0.7))
    pts = grid(shape[0], shape[1], 16, 8, (0.37, 0.81))
    got, want = both(vp, a, b, pts, win=win, max_level=3)
    check(got, want, win)
    if win == (63, 63):
        assert feature.flow_level_count(160, 144, win, 3) == 2, "one reduced level"
    assert got[1].any()


def test_points_on_at_and_beyond_the_frame(vp):
    a, b = frames(80, 96, 4, (0.8, -0.6))
    h, w = 80, 96
    pts = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1],                      # the four corner pixels
                    [40, 30], [40.5, 30.5], [40.5, 30], [40, 30.5], [10.5, 10.5],       # fractions of exactly 0 and 0.5 (window 21: half 10)
                    [-0.5, 20], [20, -0.5], [-0.5, -0.5], [w - 0.5, h - 0.5],           # just outside
                    [-11, 20], [-11.01, 20], [-12, 20], [w + 10, 20], [w + 11, 20], [20, h + 10], [20, h + 11], [20, -11], [20, -11.5],   # round the range test
                    [-500, 30], [30, 5000], [1e6, 1e6], [16777216, 3], [16777218, 3], [-16777216, -16777216],      # far outside, and the 2^24 limit
                    [np.nan, 5], [5, np.nan], [np.inf, 5], [5, -np.inf], [1e30, 5], [5, -1e30]], np.float32)
    for ml in (0, 2):
        got, want = both(vp, a, b, pts, max_level=ml)
        check(got, want, ml)
    assert not got[1][-6:].any() and not got[2][-6:].any()
    assert got[0].reshape(-1, 2)[-6:].tobytes() == pts[-6:].tobytes(), "a point that is not finite comes back as it went in"
    assert got[1][:4].any(), "a corner pixel is trackable: the window reads the reflected border"


def test_flat_region_next_to_texture_loses_points_with_err_zero(vp):
    a, b = (x.copy() for x in frames(96, 128, 5, (0.6, 0.4)))
    a[:, :64] = 90
    b[:, :64] = 90
    pts = grid(96, 128, 8, 12)
    got, want = both(vp, a, b, pts, max_level=2)
    check(got, want)
    lost = ~got[1]
    assert lost.any() and got[1].any() and not got[2][lost].any()
    got, want = both(vp, a, b, pts, max_level=2, min_eigenvals=True)
    check(got, want, "eigenvalues")
    assert (got[2][lost] < 1e-4).all()


def test_a_large_shift_takes_points_out_of_the_frame_in_mid_iteration(vp):
    a, b = frames(96, 128, 6, (17.0, 9.0))
    pts = grid(96, 128, 10, 4)
    for ml in (0, 3):
        got, want = both(vp, a, b, pts, max_level=ml, win=(9, 9))
        check(got, want, ml)
    rough = R.texture(96, 128, 7, waves=64, top=2.5)                 # unrelated fine texture: steps are large and erratic
    got, want = both(vp, a, rough, pts, max_level=0, win=(5, 5), min_eig=0.0)
    check(got, want, "rough")
    assert not want[1].all(), "no point left the frame: the case checks nothing"


@pytest.mark.parametrize("max_count", [0, 1, 2, 30, 1000, -3])
def test_max_count(vp, max_count):
    a, b = frames()
    check(*both(vp, a, b, grid(120, 160, 20), max_count=max_count, eps=0.0))


@pytest.mark.parametrize("eps", [0.0, 10.0, 50.0, -1.0])
def test_eps(vp, eps):
    a, b = frames()
    check(*both(vp, a, b, grid(120, 160, 20), eps=eps))


def test_initial_guess(vp):
    a, b = frames()
    pts = grid(120, 160, 16)
    r = np.random.default_rng(8)
    guess = (pts + np.float32(SHIFT) + r.uniform(-1.5, 1.5, pts.shape)).astype(np.float32)
    guess[3] = (np.nan, 1)
    guess[4] = (-300, 40)
    guess[5] = (3e7, 40)
    for ml in (0, 2):
        got, want = both(vp, a, b, pts, guess, max_level=ml)
        check(got, want, ml)
    assert got[0].reshape(-1, 2)[3].tobytes() == guess[3].tobytes() and not got[1][3] and not got[1][5]
    got, want = both(vp, a, b, pts, guess, max_level=1, max_count=0)
    check(got, want, "no iteration")


def test_minimum_eigenvalue_flag(vp):
    a, b = frames()
    pts = np.concatenate([grid(120, 160, 16), np.array([[-40, 3], [np.nan, 0]], np.float32)])
    got, want = both(vp, a, b, pts, min_eigenvals=True)
    check(got, want)
    assert (got[2][:-2] > 1e-4).all() and not got[2][-2:].any()
    check(*both(vp, a, b, pts, min_eigenvals=True, min_eig=1e9, max_level=1))          # every point lost, err still the eigenvalue


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_point_counts_round_the_wave(vp, n):
    a, b = frames()
    r = np.random.default_rng(n)
    pts = np.stack([r.uniform(-5, 165, n), r.uniform(-5, 125, n)], 1).astype(np.float32)
    check(*both(vp, a, b, pts, max_level=2))


def test_strided_level_0_pyramid_reuse_and_device_images(vp):
    from vision.devmat import DeviceMat
    from vision.utils import feature
    a, b = frames(96, 128, 9, (1.1, -0.9))
    c = R.texture(96, 128, 9, (2.0, -2.1))
    pts = grid(96, 128, 12, 10)
    ctx = vp.default_context()
    want_ab = R.lk_restate(a, b, pts)
    # numpy in and DeviceMat in give the same bits
    da, db = DeviceMat.from_host(ctx, a), DeviceMat.from_host(ctx, b)
    check(feature.track_points(da, db, pts), want_ab, "device images")
    check(feature.track_points(a, b, pts), want_ab, "numpy images")
    # a window of a wider device image: level 0 has a stride above its row
    wide = np.full((110, 200), 255, np.uint8)
    wide[7:103, 31:159] = a
    crop = feature.DeviceCrop(DeviceMat.from_host(ctx, wide), 31, 7, 128, 96)
    check(feature.track_points(crop, db, pts), want_ab, "strided level 0")
    # A -> B, then B -> C with B's pyramid reused
    pa, pb, pc = (feature.FlowPyramid(x) for x in (a, b, c))
    assert len(pb) == 3 and pb.shape == (96, 128)
    got_ab = feature.track_points(pa, pb, pts)
    check(got_ab, want_ab, "pyramids")
    mid = got_ab[0].reshape(-1, 2)
    check(feature.track_points(pb, pc, mid), R.lk_restate(b, c, mid), "reused pyramid")
    check(feature.track_points(b, c, mid), R.lk_restate(b, c, mid), "fresh call")
    check(feature.track_points(pa, pb, pts, max_level=1), R.lk_restate(a, b, pts, max_level=1), "a pyramid serves a smaller maxLevel")
    with pytest.raises(ValueError):
        feature.track_points(pa, pb, pts, win_size=(5, 5), max_level=5)                # more levels than the pyramids hold
    # two runs, identical bits
    again = feature.track_points(pa, pb, pts)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again, got_ab))


def test_back_check_is_the_statement_run_both_ways(vp):
    from vision.utils import feature
    a, b = (x.copy() for x in frames(96, 128, 10, (1.4, 0.9)))
    b[30:70, 40:90] = R.texture(40, 50, 11, waves=64, top=2.5)                          # a patch that does not match: tracks there do not return
    pts = grid(96, 128, 8, 6)
    t = 0.5
    fwd = R.lk_restate(a, b, pts)
    back = R.lk_restate(b, a, fwd[0])
    d = back[0].astype(np.float64) - pts.astype(np.float64)
    keep = (fwd[1] != 0) & (back[1] != 0) & ~(d[:, 0] ** 2 + d[:, 1] ** 2 > t * t)
    got = feature.track_points(a, b, pts, back_check=t)
    check(got, (fwd[0], keep, fwd[2]))
    assert keep.any() and (keep != (fwd[1] != 0)).any(), "the check clears some and keeps some"


def test_facade_shapes_flags_and_the_host_entry(vp):
    import ctypes as C
    from vision import cv2_facade as f
    a, b = frames()
    pts = grid(120, 160, 16)
    want = R.lk_restate(a, b, pts, win=(15, 11), max_level=2, max_count=10, eps=0.03)
    nxt, st, err = f.calcOpticalFlowPyrLK(a, b, pts.reshape(-1, 1, 2), None, winSize=(15, 11), maxLevel=2,
                                          criteria=(f.TERM_CRITERIA_COUNT | f.TERM_CRITERIA_EPS, 10, 0.03))
    assert nxt.shape == (len(pts), 1, 2) and st.shape == (len(pts), 1) and st.dtype == np.uint8 and err.shape == (len(pts), 1) and err.dtype == np.float32
    check((nxt, st[:, 0], err[:, 0]), want)
    want = R.lk_restate(a, b, pts, pts + 1, flags=12)                                    # criteria without bits: 30 and 0.01
    nxt, st, err = f.calcOpticalFlowPyrLK(a, b, pts, pts + 1, criteria=(0, 1, 5.0), flags=f.OPTFLOW_USE_INITIAL_FLOW | f.OPTFLOW_LK_GET_MIN_EIGENVALS)
    check((nxt, st[:, 0], err[:, 0]), want)
    # vp_lk_flow_u8: stages, builds both pyramids, runs and synchronises
    out = np.zeros((len(pts), 4), np.uint32)
    ctx = vp.default_context()
    a2, b2 = np.ascontiguousarray(a), np.ascontiguousarray(b)
    vp.check(vp.lib().vp_lk_flow_u8(ctx.handle, a2.ctypes.data, b2.ctypes.data, 160, 120, pts.ctypes.data, None, len(pts), 21, 21, 3, 30, 0.01, 0, 1e-4,
                                    out.ctypes.data), ctx.handle)
    check((out[:, :2].copy().view(np.float32), out[:, 3], out[:, 2].copy().view(np.float32)), R.lk_restate(a, b, pts))
