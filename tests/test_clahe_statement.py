"""CPU suite for the statement of cv2.equalizeHist and CLAHE (tests/clahe_restate.py): its literal-loop form and its vectorised form
agree on every kind of image and grid; the closed form of the residual's distribution equals the loop for every residual; answers
worked out by hand; and the 16 x 16 image on an 8 x 8 grid, whose weights are 0 and 0.5, produces exact rounding ties."""
import numpy as np
import pytest

import clahe_restate as R

CLIPS = [0, 1e-3, 2.0, 40.0, 1e4]
# (w, h), (tiles_x, tiles_y): divisible; not divisible in both; divisible in x only and in y only (the whole-tile quirk); one tile
GRIDS = [((64, 64), (8, 8)), ((16, 16), (8, 8)), ((48, 30), (4, 3)), ((37, 29), (4, 3)), ((40, 29), (4, 3)), ((37, 30), (4, 3)), ((9, 9), (8, 8)),
         ((23, 17), (1, 1)), ((23, 17), (1, 8)), ((23, 17), (8, 1))]


def _images(w, h):
    rng = np.random.default_rng(w * 131 + h)
    yield "random", rng.integers(0, 256, (h, w), dtype=np.uint8)
    yield "constant", np.full((h, w), 93, np.uint8)
    yield "two-valued", np.where(rng.random((h, w)) < 0.3, 200, 17).astype(np.uint8)
    yield "ramp", ((np.arange(w)[None, :] * 3 + np.arange(h)[:, None] * 5) % 256).astype(np.uint8)
    yield "narrow", rng.integers(100, 108, (h, w), dtype=np.uint8)


@pytest.mark.parametrize("size,grid", GRIDS)
def test_the_two_forms_of_clahe_agree(size, grid):
    w, h = size
    for name, img in _images(w, h):
        for clip in CLIPS:
            a, b = R.clahe(img, clip, grid), R.clahe_loops(img, clip, grid)
            assert a.dtype == np.uint8 and a.shape == (h, w) and np.array_equal(a, b), (name, clip)


@pytest.mark.parametrize("size", [s for s, _ in GRIDS])
def test_the_two_forms_of_equalize_hist_agree(size):
    w, h = size
    for name, img in _images(w, h):
        assert np.array_equal(R.equalize_hist(img), R.equalize_hist_loops(img)), name


def test_geometry_pads_both_dimensions_whenever_either_fails_to_divide():
    assert R.geometry(64, 64, 8, 8) == (64, 64, 8, 8)
    assert R.geometry(37, 29, 4, 3) == (40, 30, 10, 10)
    assert R.geometry(40, 29, 4, 3) == (44, 30, 11, 10)          # 40 divides by 4 and still grows by a whole 4
    assert R.geometry(37, 30, 4, 3) == (40, 33, 10, 11)
    assert R.geometry(9, 9, 8, 8) == (16, 16, 2, 2)
    assert R.geometry(1920, 1080, 8, 8) == (1920, 1080, 240, 135)


def test_clip_count_truncates_in_double_and_is_at_least_one():
    assert R.clip_count(0, 64) == 0 and R.clip_count(-3.0, 64) == 0
    assert R.clip_count(1e-3, 64) == 1
    assert R.clip_count(40.0, 64) == 10 and R.clip_count(2.0, 32400) == 253 and R.clip_count(1e4, 4) == 156


def test_residual_closed_form_is_the_literal_loop_and_the_loop_never_runs_out_of_bins():
    for residual in range(1, 256):
        bins, ran_out = R.residual_bins_loop(residual)
        assert not ran_out and len(bins) == residual, residual
        assert bins == R.residual_bins_closed(residual), residual


def test_constant_image_without_clipping_is_255_everywhere():
    for (w, h), grid in GRIDS:
        img = np.full((h, w), 41, np.uint8)
        assert (R.clahe(img, 0, grid) == 255).all() and (R.clahe_loops(img, 0, grid) == 255).all()


def test_constant_tile_with_clip_limit_40_by_hand():
    """One 8 x 8 tile of value v: 64 pixels in bin v.  clip = int(40 * 64 / 256) = 10, so 54 are cut; 54 / 256 = 0 to every bin, residual
    54, step = 256 / 54 = 4: bins 0, 4, ..., 212 get one each.  Table entry i = rint(float32(prefix sum) * float32(255 / 64))."""
    for v in (0, 2, 100, 212, 213, 255):
        hist = np.zeros(256, np.int64)
        hist[v] = 10
        hist[0:213:4] += 1
        assert hist.sum() == 64
        want = np.clip(np.rint(np.cumsum(hist).astype(np.float32) * (np.float32(255) / np.float32(64))), 0, 255).astype(np.uint8)
        img = np.full((8, 8), v, np.uint8)
        assert np.array_equal(R.tile_luts(img, 40.0, (1, 1))[0, 0], want)
        assert np.array_equal(R.tile_lut_loops(img.ravel(), 10, 64), want)
        # one tile: both neighbours are that tile, the weights sum to 1 up to rounding
        assert (R.clahe(img, 40.0, (1, 1)) == want[v]).all() and (R.clahe_loops(img, 40.0, (1, 1)) == want[v]).all()


def test_equalize_hist_known_answers():
    for v in (0, 7, 255):
        img = np.full((5, 9), v, np.uint8)
        assert (R.equalize_hist(img) == v).all() and (R.equalize_hist_loops(img) == v).all()       # the single-value early return
    img = np.full((6, 10), 50, np.uint8)
    img[:2] = 180                                        # 40 pixels at 50, 20 at 180: the lowest value maps to 0, scale = 255 / 20
    want = np.where(img == 50, 0, 255).astype(np.uint8)
    assert np.array_equal(R.equalize_hist(img), want) and np.array_equal(R.equalize_hist_loops(img), want)
    img = np.zeros((4, 4), np.uint8)
    img.ravel()[:] = [10] * 4 + [20] * 4 + [30] * 8      # scale = 255 / 12: 20 -> rint(85) = 85, 30 -> 255
    want = np.array([0] * 4 + [85] * 4 + [255] * 8, np.uint8).reshape(4, 4)
    assert np.array_equal(R.equalize_hist(img), want) and np.array_equal(R.equalize_hist_loops(img), want)


def test_two_by_two_tiles_give_exact_rounding_ties():
    """16 x 16 on an 8 x 8 grid: tiles of 2 x 2, x / 2 - 0.5 has fraction 0 or 0.5, so the blend of two table entries that differ by an odd
    amount is exactly k + 0.5: rint must round it to even.  Some such pixels must occur, or the case tests nothing."""
    rng = np.random.default_rng(16)
    img = rng.integers(0, 256, (16, 16), dtype=np.uint8)
    luts = R.tile_luts(img, 40.0, (8, 8)).astype(np.float64)
    got, got_loops = R.clahe(img, 40.0, (8, 8)), R.clahe_loops(img, 40.0, (8, 8))
    ties = 0
    for y in range(16):
        for x in range(16):
            fx, fy = x / 2 - 0.5, y / 2 - 0.5
            tx1, ty1 = int(np.floor(fx)), int(np.floor(fy))
            xa, ya = fx - tx1, fy - ty1
            assert xa in (0.0, 0.5) and ya in (0.0, 0.5)
            tx2, ty2, tx1, ty1 = min(tx1 + 1, 7), min(ty1 + 1, 7), max(tx1, 0), max(ty1, 0)
            v = img[y, x]
            exact = (luts[ty1, tx1, v] * (1 - xa) + luts[ty1, tx2, v] * xa) * (1 - ya) + (luts[ty2, tx1, v] * (1 - xa) + luts[ty2, tx2, v] * xa) * ya
            if exact * 2 % 2 == 1:
                ties += 1
                even = int(exact - 0.5) if int(exact - 0.5) % 2 == 0 else int(exact + 0.5)
                assert got[y, x] == even == got_loops[y, x], (x, y, exact)
    assert ties > 0


def test_fused_products_change_few_pixels_but_some():
    """the open point of DESIGN.md: a fused multiply-add in the blend is a different function"""
    import frames as F
    grey = np.ascontiguousarray(F.s1_buoy(0, 1920, 1080)[:, :, 1])
    plain, fused = R.clahe(grey, 2.0, (8, 8)), R.clahe_fused_f64(grey, 2.0, (8, 8))
    diff = int((plain != fused).sum())
    assert 0 < diff < grey.size // 1000, diff
    assert int(np.abs(plain.astype(int) - fused.astype(int)).max()) == 1
