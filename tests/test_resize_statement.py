"""The statement of cv2.resize INTER_LINEAR on 8-bit images (resize_restate.py) checked on its own, without a GPU: against float64
bilinear interpolation, on the cases whose answer is known in closed form, on a small case worked by hand, and on the two readings of
resize.cpp that the kernels used to get wrong (the float32 scale and clamped row weights)."""
import numpy as np
import pytest

import resize_restate as RR

# (sh, sw) -> (dh, dw) pairs whose tables differ between the float32-scale / clamped-row reading and resize.cpp's
CHANGED = [((1080, 1920), (768, 1366)), ((1080, 1920), (2048, 2048)), ((360, 640), (1080, 1920)), ((480, 480), (640, 640)),
           ((90, 160), (512, 512)), ((100, 50), (99, 51))]
# exact halvings and ratios exact in float32, downscaling: both readings agree
UNCHANGED = [((1080, 1920), (360, 640)), ((1080, 1920), (512, 512)), ((720, 1280), (360, 640)), ((1080, 1920), (540, 960))]


def _bilinear64(img, dw, dh, scale_x, scale_y):
    """Half-pixel-centre bilinear interpolation in float64 with replicated borders: source coordinate (d + 0.5) * scale - 0.5,
    clamped into [0, size - 1]."""
    def axis(n, scale, size):
        c = np.clip((np.arange(n) + 0.5) * scale - 0.5, 0, size - 1)
        i0 = np.floor(c).astype(np.int64)
        return i0, np.minimum(i0 + 1, size - 1), c - i0
    sh, sw = img.shape[:2]
    x0, x1, wx = axis(dw, scale_x, sw)
    y0, y1, wy = axis(dh, scale_y, sh)
    f = img.astype(np.float64)
    top = f[y0][:, x0] * (1 - wx)[None, :, None] + f[y0][:, x1] * wx[None, :, None]
    bot = f[y1][:, x0] * (1 - wx)[None, :, None] + f[y1][:, x1] * wx[None, :, None]
    return top * (1 - wy)[:, None, None] + bot * wy[:, None, None]


def _sweep(n=200, seed=11):
    rng = np.random.default_rng(seed)
    side = lambda: int(np.exp(rng.uniform(0, np.log(300.5))))   # noqa: E731
    return [((side(), side()), (side(), side()), (1, 3, 4)[i % 3]) for i in range(n)]


def test_within_one_grey_level_of_float64_bilinear():
    """dsize form over a seeded sweep, fx / fy form over seeded factors: never more than one grey level from float64 bilinear."""
    rng = np.random.default_rng(12)
    worst = 0.0
    for (sw, sh), (dw, dh), cn in _sweep():
        img = rng.integers(0, 256, (sh, sw, cn), dtype=np.uint8)
        got = RR.resize(img, (dw, dh))
        worst = max(worst, np.abs(got - _bilinear64(img, dw, dh, sw / dw, sh / dh)).max())
    for (sw, sh), _, cn in _sweep(60, seed=13):
        fx, fy = np.exp(rng.uniform(np.log(0.1), np.log(4), 2))
        dw, dh = RR.saturate_int(sw * fx), RR.saturate_int(sh * fy)
        if dw < 1 or dh < 1 or (RR.area_fast_2(1 / fx, 1 / fy) and (sw != 2 * dw or sh != 2 * dh)):
            continue
        img = rng.integers(0, 256, (sh, sw, cn), dtype=np.uint8)
        got = RR.resize(img, None, fx, fy)
        ref = img if (dw, dh) == (sw, sh) else _bilinear64(img, dw, dh, 1 / fx, 1 / fy)
        worst = max(worst, np.abs(got - ref).max())
    assert worst <= 1.0


def test_constant_images_stay_constant():
    for (sw, sh), (dw, dh), cn in _sweep(120, seed=14):
        for v in (0, 1, 2, 127, 128, 254, 255):
            img = np.full((sh, sw, cn), v, np.uint8)
            assert (RR.resize(img, (dw, dh)) == v).all(), ((sw, sh), (dw, dh), v)


def test_identity_is_a_copy():
    img = np.random.default_rng(15).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    out = RR.resize(img, (53, 37))
    assert np.array_equal(out, img) and out is not img and not np.shares_memory(out, img)
    # the fx / fy form copies whenever the rounded size is the source's, whatever the factor
    assert np.array_equal(RR.resize(img, None, 1.009, 0.99), img)     # 53.48 -> 53, 36.63 -> 37
    gray = img[:, :, 0].copy()
    assert np.array_equal(RR.resize(gray, (53, 37)), gray)


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_exact_halving_is_the_2x2_average(cn):
    rng = np.random.default_rng(16 + cn)
    for h, w in ((2, 2), (2, 300), (64, 90), (300, 2)):
        img = rng.integers(0, 256, (h, w, cn), dtype=np.uint8)
        cells = img.astype(np.int64).reshape(h // 2, 2, w // 2, 2, cn).sum(axis=(1, 3))
        exp = (cells + 2) // 4
        assert np.array_equal(RR.resize(img, (w // 2, h // 2)), exp)
        assert np.array_equal(RR.resize(img, None, 0.5, 0.5), exp)
    # scale 2 on one axis only is not area-fast: bilinear at the half-pixel, which is the pair average with 11-bit rounding
    img = rng.integers(0, 256, (10, 40, cn), dtype=np.uint8)
    assert not RR.area_fast_2(2.0, 10 / 7)
    out = RR.resize(img, (20, 7))
    assert np.abs(out - _bilinear64(img, 20, 7, 2.0, 10 / 7)).max() <= 1


def test_partial_area_cell_is_not_restated():
    img = np.zeros((101, 100, 3), np.uint8)
    assert RR.area_fast_2(1 / 0.5, 1 / 0.5)
    with pytest.raises(NotImplementedError):
        RR.resize(img, None, 0.5, 0.5)


def test_unchanged_axis_is_interpolation_along_the_other():
    """dh == sh: every output row is its own source row interpolated along x (rows may be permuted freely), and the vertical pass
    reduces to ((S >> 9) + 2) >> 2 of the horizontal sums.  The same for dw == sw along y."""
    rng = np.random.default_rng(17)
    for (sw, sh), (dw, _), cn in _sweep(60, seed=18):
        img = rng.integers(0, 256, (sh, sw, cn), dtype=np.uint8)
        out = RR.resize(img, (dw, sh))
        perm = rng.permutation(sh)
        assert np.array_equal(RR.resize(img[perm], (dw, sh)), out[perm])
        if dw != sw:
            xofs, ialpha, xmax = RR.column_table(dw, sw, 1 / (dw / sw))
            S = RR.hresize(img, xofs, ialpha, xmax)
            assert np.array_equal(out, ((S >> 9) + 2) >> 2)
        out = RR.resize(img, (sw, dw))
        perm = rng.permutation(sw)
        assert np.array_equal(RR.resize(img[:, perm], (sw, dw)), out[:, perm])


def test_two_by_three_to_five_by_seven_by_hand():
    """2x3 -> 5x7 (h x w).  scale_x = 1 / (7 / 3), scale_y = 1 / (5 / 2) = 0.4.
    Columns: fx = (dx + 0.5) * 3/7 - 0.5 = -0.286, 0.143, 0.571, 1.0, 1.429, 1.857, 2.286; the first clamps to (0, fx 0), the last to
    (sw-1, fx 0); weights cvRound((1 - f) * 2048), cvRound(f * 2048).
    Rows: fy = (dy + 0.5) * 0.4 - 0.5 = -0.3, 0.1, 0.5, 0.9, 1.3: yofs -1, 0, 0, 0, 1 with fy 0.7, 0.1, 0.5, 0.9, 0.3 - not clamped."""
    xofs, ialpha, xmax, yofs, ibeta = RR.tables(3, 2, 7, 5, 7 / 3, 5 / 2)
    assert xofs.tolist() == [0, 0, 0, 1, 1, 1, 2] and xmax == 6
    assert ialpha.tolist() == [[2048, 0], [1755, 293], [878, 1170], [2048, 0], [1170, 878], [293, 1755], [2048, 0]]
    assert yofs.tolist() == [-1, 0, 0, 0, 1]
    assert ibeta.tolist() == [[614, 1434], [1843, 205], [1024, 1024], [205, 1843], [1434, 614]]
    src = np.array([[0, 63, 200], [50, 150, 250]], np.uint8)
    out = RR.resize(src, (7, 5))
    # first row, dx = 4: S = 63 * 1170 + 200 * 878 = 249310, S >> 4 = 15581; both rows clip to row 0 and keep (614, 1434):
    # (614 * 15581) >> 16 = 145, (1434 * 15581) >> 16 = 340, (145 + 340 + 2) >> 2 = 121.  Clamped weights (2048, 0) would give
    # (2048 * 15581) >> 16 = 486, (486 + 2) >> 2 = 122.
    assert out[0].tolist() == [0, 9, 36, 63, 121, 180, 200]
    # last row, dx = 1: row 1 twice with (1434, 614): S = 50 * 1755 + 150 * 293 = 131700, S >> 4 = 8231,
    # (1434 * 8231) >> 16 = 180, (614 * 8231) >> 16 = 77, (180 + 77 + 2) >> 2 = 64
    assert out[4, 1] == 64
    # middle row (fy 0.5 between rows 0 and 1), dx = 0: ((1024 * (0 >> 4)) >> 16) + ((1024 * ((50 * 2048) >> 4)) >> 16) = 0 + 100
    assert out[2, 0] == (0 + 100 + 2) >> 2


def _tables_differ(sh, sw, dh, dw):
    new_x = RR.column_table(dw, sw, 1.0 / (dw / sw))[:2]
    new_y = RR.row_table(dh, 1.0 / (dh / sh))
    old_x = RR.column_table(dw, sw, float(np.float32(sw / dw)))[:2]
    old_y = RR.column_table(dh, sh, float(np.float32(sh / dh)))[:2]
    same = lambda a, b: np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])   # noqa: E731
    return not same(new_x, old_x), not same(new_y, old_y)


@pytest.mark.parametrize("src,dst", CHANGED)
def test_float32_scale_and_clamped_rows_change_the_tables(src, dst):
    """Why the kernels changed: for these sizes the float32 scale or the clamped row weights give other tables (and other pixels)."""
    dx, dy = _tables_differ(src[0], src[1], dst[0], dst[1])
    assert dx or dy
    if dst[0] > src[0]:
        # an upscale: the first row sits above row 0 (yofs -1) and keeps a non-trivial weight pair
        yofs, ibeta = RR.row_table(dst[0], 1.0 / (dst[0] / src[0]))
        assert yofs[0] == -1 and ibeta[0, 1] > 0 and ibeta[-1, 1] > 0


@pytest.mark.parametrize("src,dst", UNCHANGED)
def test_exact_float32_ratios_agree(src, dst):
    assert _tables_differ(src[0], src[1], dst[0], dst[1]) == (False, False)


def test_float32_scale_alone_changes_1366_columns():
    assert _tables_differ(1080, 1920, 768, 1366)[0]
    assert _tables_differ(100, 50, 99, 51)[1]


def test_fx_fy_size_rounds_half_to_even():
    """saturate_cast<int>(cols * fx) is cvRound: half to even, and the scale stays 1 / fx."""
    assert RR.geometry(101, 3, None, 0.5, 0.5)[:2] == (50, 2)
    assert RR.geometry(103, 5, None, 0.5, 0.5)[:2] == (52, 2)
    assert RR.geometry(5, 7, None, 0.3, 0.5)[:2] == (2, 4)     # 1.5 -> 2, 3.5 -> 4
    assert RR.geometry(10, 10, None, 0.25, 0.45)[:2] == (2, 4)  # 2.5 -> 2, 4.5 -> 4
    dw, dh, inv_x, inv_y = RR.geometry(101, 60, None, 0.5, 0.5)
    assert (inv_x, inv_y) == (0.5, 0.5) and RR.area_fast_2(1 / inv_x, 1 / inv_y)
    assert not RR.area_fast_2(101 / 50, 60 / 30)                  # the dsize form of the same sizes is bilinear
    with pytest.raises(ValueError):
        RR.geometry(3, 3, None, 0.1, 0.1)                         # empty destination
    with pytest.raises(ValueError):
        RR.geometry(3, 3, None, 0.0, 1.0)
