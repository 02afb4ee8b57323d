"""The numpy statement of cv2.calcOpticalFlowPyrLK (tests/flow_restate.py, the oracle of tests/test_gpu_flow.py) against facts that can
be checked by hand.  CPU only."""
import numpy as np

import flow_restate as R


def test_identical_frames_one_iteration_err_zero_and_the_same_bits():
    """Coordinates that are multiples of 1/4 keep every float32 step exact ((p - halfWin) + halfWin == p at every level), so the
    positions come back bit for bit; the first step is 0 and ends the loop."""
    a = R.texture(90, 110, 2)
    ys, xs = np.mgrid[12:80:9, 12:100:9]
    pts = np.stack([xs.ravel() + 0.25, ys.ravel() + 0.5], 1).astype(np.float32)
    for max_level in (0, 2):
        info = {}
        nxt, status, err = R.lk_restate(a, a, pts, max_level=max_level, info=info)
        assert nxt.tobytes() == pts.tobytes() and status.all() and not err.any()
        assert (info["iters"] == 1).all() and info["levels"] == max_level + 1


def test_weights_at_integer_positions_and_at_the_half_pixel_ties():
    f = np.float32
    assert R.weights(f(0), f(0)) == (16384, 0, 0, 0)
    assert R.weights(f(0.5), f(0.5)) == (4096, 4096, 4096, 4096)
    assert R.weights(f(0.5), f(0)) == (8192, 8192, 0, 0) and R.weights(f(0), f(0.5)) == (8192, 0, 8192, 0)
    for a in (0.0, 0.25, 0.5, 0.75, 2.0 ** -15, 1 - 2.0 ** -15, 0.3, 0.7):          # 2^-15 * 2^14 = 0.5: a tie, rounded to even
        for b in (0.0, 0.5, 2.0 ** -15, 1 - 2.0 ** -15, 0.9):
            w = R.weights(f(a), f(b))
            assert sum(w) == 1 << 14 and min(w[:3]) >= 0, (a, b, w)
    assert R.weights(f(2.0 ** -15), f(0)) == (16384, 0, 0, 0), "16383.5 rounds to the even 16384, 0.5 to the even 0"
    img = np.arange(40 * 50, dtype=np.int64).reshape(40, 50) % 251
    L = R._Level(img.astype(np.uint8), img.astype(np.uint8), 5, 3)
    got = L.sample(L.I, 7, 9, R.weights(f(0), f(0)), R.W_BITS - 5)
    assert (got == 32 * img[9:12, 7:12]).all(), "at an integer position the sample is 32 * src"


def test_descale_and_scharr_by_hand():
    assert [int(R.descale(np.int64(v), 9)) for v in (0, 255, 256, 767, 768, -256, -257)] == [0, 0, 1, 1, 2, 0, -1]
    ramp = np.tile(np.arange(8, dtype=np.uint8) * 3, (6, 1))
    ix, iy = R.scharr_deriv(ramp)
    assert (ix[:, 1:-1] == 16 * 2 * 3).all() and (ix[:, [0, -1]] == 0).all() and not iy.any(), "a ramp of 3 per pixel; reflect-101 makes the edge flat"
    ix, iy = R.scharr_deriv(ramp.T.copy())
    assert (iy[1:-1] == 96).all() and not ix.any()


def test_a_flat_image_is_lost_with_err_zero():
    flat = np.full((60, 70), 131, np.uint8)
    pts = np.array([[20, 20], [35.5, 30.25]], np.float32)
    nxt, status, err = R.lk_restate(flat, flat, pts)
    assert not status.any() and not err.any() and nxt.tobytes() == pts.tobytes()
    nxt, status, err = R.lk_restate(flat, flat, pts, flags=R.OPTFLOW_LK_GET_MIN_EIGENVALS)
    assert not status.any() and not err.any(), "S = 0: the minimum eigenvalue is exactly 0"


def test_level_rule():
    assert R.level_count(100, 90, 21, 21, 5) == 3, "100, 50, 25 exist; the 13-wide level falls out: the effective maxLevel is 2"
    assert [l.shape for l in R.build_levels(np.zeros((90, 100), np.uint8), 21, 21, 5)] == [(90, 100), (45, 50), (23, 25)]
    assert R.level_count(100, 90, 21, 21, 1) == 2 and R.level_count(22, 22, 21, 21, 3) == 1 and R.level_count(21, 40, 21, 21, 3) == 0
    assert R.level_count(43, 43, 21, 21, 3) == 2 and R.level_count(42, 42, 21, 21, 3) == 1, "(43 + 1) / 2 = 22 > 21, 42 / 2 = 21 is not"


def test_points_that_are_not_finite_or_beyond_the_limit_are_echoed():
    a = R.texture(60, 70, 3)
    pts = np.array([[np.nan, 3], [3, np.inf], [1e30, 3], [16777218, 3], [30, 30]], np.float32)
    nxt, status, err = R.lk_restate(a, a, pts)
    assert nxt.tobytes() == pts.tobytes() and status.tolist() == [0, 0, 0, 0, 1] and not err.any()
    guess = np.array([[1, 1], [2, 2], [3, 3], [4, 4], [-np.inf, 0]], np.float32)
    nxt, status, err = R.lk_restate(a, a, pts, guess, flags=R.OPTFLOW_USE_INITIAL_FLOW)
    assert nxt.tobytes() == guess.tobytes() and not status.any()


def test_a_known_sub_pixel_translation_is_recovered():
    """A band-limited texture sampled at (x - 2.3, y + 1.6): interior points must come back shifted by (2.3, -1.6).  Measured worst
    error of the statement on this CPU over the three level counts: 0.0144 pixels (the images are quantised to bytes and the
    derivative window is that of the first image only); the bound is twice that.  It guards the statement against a wrong sign or
    a swapped axis - the gate for the GPU is equality with the statement, not this tolerance."""
    shift = (2.3, -1.6)
    a, b = R.texture(120, 160, 1), R.texture(120, 160, 1, shift)
    ys, xs = np.mgrid[30:90:12, 30:130:12]
    pts = np.stack([xs.ravel() + 0.25, ys.ravel() + 0.5], 1).astype(np.float32)
    worst = 0.0
    for max_level in (0, 1, 3):
        nxt, status, err = R.lk_restate(a, b, pts, max_level=max_level)
        assert status.all()
        worst = max(worst, float(np.abs(nxt - pts - np.float32(shift)).max()))
    print("worst error", worst)
    assert worst <= 2 * 0.0144
