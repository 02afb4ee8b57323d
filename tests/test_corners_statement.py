"""CPU statement of the corner operators (tests/corners_restate.py): answers worked by hand, the bound that keeps
the structure tensor in int32, the symmetries of the response map, and the equivalence of the contract's 3 x 3 test with the
threshold / dilate / compare wording of featureselect.cpp."""
import numpy as np
import pytest

import corners_restate as R


def _bright_pixel():
    img = np.zeros((5, 5), np.uint8)
    img[2, 2] = 255
    return img


def test_one_bright_pixel_by_hand():
    """p = 255 at the centre of a 5 x 5 image.  Dx is p (1, 2, 1) down column 1 and the negative down column 3, Dy the transpose; so
    Pxx = Pyy sum to 12 p^2 over the centre's 3 x 3 window and Pxy (+p^2, -p^2, -p^2, +p^2 at the four diagonal pixels) to 0: the two
    eigenvalues are equal, L = 12 p^2, and with s = 1 / (12 * 255) the response is 12 p^2 s^2 = 1 / 12.  At (1, 1) the window holds
    Sxx = Syy = 5 p^2 and Sxy = p^2: L = 5 p^2 - p^2 = 4 p^2, a third of the centre's."""
    img = _bright_pixel()
    p2 = 255.0 * 255.0
    s = 1.0 / (4.0 * 3 * 255.0)
    sxx, sxy, syy = R.structure_tensor(img, 3)
    assert (sxx[2, 2], sxy[2, 2], syy[2, 2]) == (12 * 65025, 0, 12 * 65025)
    assert (sxx[1, 1], sxy[1, 1], syy[1, 1]) == (5 * 65025, 65025, 5 * 65025)
    assert (sxx[1, 2], sxy[1, 2], syy[1, 2]) == (10 * 65025, 0, 6 * 65025)
    resp = R.min_eigen_val(img, 3)
    assert resp.dtype == np.float32 and resp.shape == (5, 5)
    assert resp[2, 2] == np.float32((12.0 * p2) * (s * s)) and abs(float(resp[2, 2]) - 1.0 / 12.0) < 1e-8
    assert resp[1, 1] == np.float32((4.0 * p2) * (s * s)) and resp[1, 2] == np.float32((6.0 * p2) * (s * s))
    assert np.array_equal(resp, resp.T) and np.array_equal(resp, resp[::-1, ::-1])
    hr = R.harris(img, 3, 0.04)
    a = 12.0 * p2
    assert hr[2, 2] == np.float32(((a * a - 0.0) - 0.04 * ((a + a) * (a + a))) * ((s * s) * (s * s)))
    for q in (0.01, 0.5, 0.999):
        got = R.good_features(img, 0, q, 0)
        assert got.dtype == np.float32 and got.shape == (1, 1, 2) and got.tolist() == [[[2.0, 2.0]]]
    assert R.good_features(img[:2], 0) is None and R.good_features(img[:, :2], 0) is None, "no interior pixel"
    assert R.good_features(np.full((5, 5), 77, np.uint8), 0) is None, "a constant image has no corner"


@pytest.mark.parametrize("border", (R.REFLECT_101, R.REPLICATE, R.REFLECT))
@pytest.mark.parametrize("block", (1, 2, 3, 4, 7, 31))
def test_a_straight_edge_is_exactly_zero(block, border):
    """a vertical step: Dy = 0 everywhere, so Syy = Sxy = 0, a = Sxx / 2 and L = a - sqrt(a a) = +0.0 exactly - sqrt is correctly
    rounded and sqrt(RN(a a)) = a.  (Under a constant border the image's own outline is an edge with corners.)"""
    img = np.zeros((9, 12), np.uint8)
    img[:, 6:] = 255
    resp = R.min_eigen_val(img, block, border)
    assert resp.tobytes() == np.zeros((9, 12), np.float32).tobytes(), "not +0.0 everywhere"
    assert R.good_features(img, 0, 0.01, 0, block=block) is None
    assert R.min_eigen_val(img.T.copy(), block, border).tobytes() == resp.T.tobytes()


def test_checkerboard_plateau_is_kept_whole_in_larger_index_first_order():
    """2 x 2 cells of 4 pixels: the crossing lies between pixels (3, 3), (3, 4), (4, 3), (4, 4), which the pattern's symmetries map onto
    each other (an inversion of the colours changes no product), so their integer sums and responses are equal: a plateau, kept whole,
    ordered by raster index y * 8 + x descending: 36, 35, 28, 27."""
    img = np.zeros((8, 8), np.uint8)
    img[:4, 4:] = 255
    img[4:, :4] = 255
    resp = R.min_eigen_val(img, 3)
    top = resp[3, 3]
    assert top > 0 and resp[3, 4] == top and resp[4, 3] == top and resp[4, 4] == top and (resp <= top).all()
    assert int((resp == top).sum()) == 4
    got = R.good_features(img, 0, 0.999, 0)
    assert got.tolist() == [[[4.0, 4.0]], [[3.0, 4.0]], [[4.0, 3.0]], [[3.0, 3.0]]]
    assert R.good_features(img, 2, 0.999, 0).tolist() == [[[4.0, 4.0]], [[3.0, 4.0]]]
    assert R.good_features(img, 0, 0.999, 1).tolist() == got.tolist(), "two pixels are never closer than 1"
    assert R.good_features(img, 0, 0.999, 1.2).tolist() == [[[4.0, 4.0]], [[3.0, 3.0]]], "the diagonal neighbour is sqrt(2) away"
    assert R.good_features(img, 0, 0.999, 1.5).tolist() == [[[4.0, 4.0]]]
    mask = np.full((8, 8), 255, np.uint8)
    mask[4, 4] = 0
    assert R.good_features(img, 0, 0.999, 0, mask=mask).tolist() == [[[3.0, 4.0]], [[4.0, 3.0]], [[3.0, 3.0]]]


def test_int32_holds_every_box_sum_of_every_admitted_block_size():
    assert R.MAX_DERIV == 4 * 255 and R.MAX_BLOCK == 31
    for block in range(1, R.MAX_BLOCK + 1):
        assert block * block * R.MAX_DERIV * R.MAX_DERIV < 2 ** 31
    assert 32 * 32 * R.MAX_DERIV * R.MAX_DERIV < 2 ** 31 <= 46 * 46 * R.MAX_DERIV * R.MAX_DERIV, "and where the bound ends"
    rng = np.random.default_rng(5)
    for img in (rng.integers(0, 256, (13, 17), dtype=np.uint8), rng.choice(np.array([0, 255], np.uint8), (13, 17)),
                (np.indices((13, 17)).sum(0) % 2 * 255).astype(np.uint8)):
        for border in R.BORDERS:
            dx, dy = R.sobel_pair(img, border)
            assert max(abs(dx).max(), abs(dy).max()) <= R.MAX_DERIV
            for t in R.structure_tensor(img, 31, border):
                assert abs(t).max() < 2 ** 31
    edge = np.zeros((40, 40), np.uint8)                 # a full step reaches the largest derivative
    edge[:, 20:] = 255
    assert abs(R.sobel_pair(edge, R.REFLECT_101)[0]).max() == R.MAX_DERIV


@pytest.mark.parametrize("block", (1, 2, 3, 4, 7))
def test_transpose_and_rotation_permute_the_response(block):
    rng = np.random.default_rng(block)
    img = rng.integers(0, 256, (11, 14), dtype=np.uint8)
    for border in R.BORDERS:
        for fn in (lambda m: R.min_eigen_val(m, block, border), lambda m: R.harris(m, block, 0.04, border)):
            ref = fn(img)
            assert fn(np.ascontiguousarray(img.T)).tobytes() == np.ascontiguousarray(ref.T).tobytes()
            if block % 2:                               # an even window's anchor is not the centre: a flip moves it
                assert fn(np.ascontiguousarray(np.rot90(img))).tobytes() == np.ascontiguousarray(np.rot90(ref)).tobytes()
                assert fn(np.ascontiguousarray(img[::-1])).tobytes() == np.ascontiguousarray(ref[::-1]).tobytes()


def test_the_3x3_test_is_featureselects_threshold_dilate_compare():
    """brute force on small maps with many ties, zeros and negative values, thresholds made as the pipeline makes them.  The two wordings
    agree for qualityLevel <= 1 (cv2's documented range): then t >= 0 whenever anything is above it, and a neighbour the threshold
    zeroed can never beat a value above t."""
    rng = np.random.default_rng(11)
    seen = 0
    for trial in range(300):
        h, w = int(rng.integers(3, 8)), int(rng.integers(3, 8))
        vals = np.array([-2.0, -0.5, 0.0, 0.25, 0.5, 1.0, 3.0], np.float32)
        resp = rng.choice(vals[int(rng.integers(0, 3)):int(rng.integers(3, 8))], (h, w)).astype(np.float32)
        mask = None if trial % 3 else rng.choice(np.array([0, 255], np.uint8), (h, w))
        for q in (0.01, 0.3, 0.5, 1.0):
            _, t = R.threshold_of(resp, q, mask)
            if t is None:
                continue
            a, b = R.candidates(resp, t, mask), R.candidates_cv2(resp, t, mask)
            assert [(y, x) for _, y, x in a] == [(y, x) for _, y, x in b], (resp, t, mask)
            seen += len(a)
    assert seen > 300, "the maps exercised the test"


def test_selection_order_and_distance():
    cands = [(np.float32(1.0), 1, 1), (np.float32(2.0), 1, 5), (np.float32(1.0), 3, 2), (np.float32(2.0), 2, 5), (np.float32(0.5), 5, 5)]
    w = 8
    assert R.select(cands, w, 0, 0) == [(5, 2), (5, 1), (2, 3), (1, 1), (5, 5)]
    assert R.select(cands, w, 3, 0.5) == [(5, 2), (5, 1), (2, 3)]
    assert R.select(cands, w, 0, 1) == [(5, 2), (5, 1), (2, 3), (1, 1), (5, 5)]
    assert R.select(cands, w, 0, 3) == [(5, 2), (2, 3), (5, 5)], "(5, 1) is 1 from (5, 2); (1, 1) is sqrt(5) from (2, 3); (5, 5) is exactly 3 away"
    assert R.select(cands, w, 0, 3.0001) == [(5, 2), (2, 3)]
    assert R.select(cands, w, 0, 100) == [(5, 2)]
    assert R.select(cands, w, 1, 100) == [(5, 2)]
