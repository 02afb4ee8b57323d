"""CPU suite for the statement of cv2.distanceTransform / cv2.minMaxLoc (tests/dist_restate.py): the brute-force
minimum and the separable transform agree, hand answers agree with both, and min_max_loc follows cv2's rules on ties, masks, NaN and
infinities.  Every comparison is exact."""
import numpy as np
import pytest

import dist_restate as R

INF = np.float32(np.inf)


def _all_ways(img, metric):
    a = R.brute(img, metric)
    assert np.array_equal(a, R.separable(img, metric)) and np.array_equal(a, R.separable_fast(img, metric)) and np.array_equal(a, R.reference(img, metric))
    return a


@pytest.mark.parametrize("density", (0.005, 0.1, 0.5, 0.99))
def test_the_two_statements_agree_on_random_masks(density):
    rng = np.random.default_rng(int(density * 1000))
    for h, w in ((1, 1), (1, 17), (23, 1), (7, 9), (31, 40), (40, 40)):
        img = np.where(rng.random((h, w)) < density, 0, 255).astype(np.uint8)
        for metric in R.METRICS:
            ints = _all_ways(img, metric)
            assert R.finish(ints, metric).dtype == np.float32
            if metric == R.L1:
                assert R.finish(ints, metric, np.uint8).dtype == np.uint8


def test_one_zero_at_the_centre_of_5_by_5():
    img = np.full((5, 5), 255, np.uint8)
    img[2, 2] = 0
    d = np.abs(np.arange(5) - 2)
    dy, dx = d[:, None], d[None, :]
    assert np.array_equal(_all_ways(img, R.L2), dy * dy + dx * dx)
    assert np.array_equal(_all_ways(img, R.L1), dy + dx)
    assert np.array_equal(_all_ways(img, R.C), np.maximum(dy, dx))
    l2 = R.distance_transform(img, R.L2)
    assert l2[2, 2] == 0 and l2[2, 4] == 2 and l2[0, 0].tobytes() == np.sqrt(np.float32(8)).tobytes() and l2[1, 1].tobytes() == np.sqrt(np.float32(2)).tobytes()
    assert R.distance_transform(img, R.L1, np.uint8).tolist() == (dy + dx).tolist()


def test_one_zero_at_the_origin_of_a_row_and_of_a_column():
    for shape in ((1, 9), (9, 1)):
        img = np.full(shape, 255, np.uint8)
        img[0, 0] = 0
        ramp = np.arange(9).reshape(shape)
        assert np.array_equal(_all_ways(img, R.L2), ramp * ramp)
        assert np.array_equal(_all_ways(img, R.L1), ramp) and np.array_equal(_all_ways(img, R.C), ramp)
        assert R.distance_transform(img, R.L2).tobytes() == ramp.astype(np.float32).tobytes()


def test_all_zero_no_zero_and_a_column_without_zeros():
    for metric in R.METRICS:
        assert not _all_ways(np.zeros((6, 7), np.uint8), metric).any()
        assert (_all_ways(np.full((6, 7), 255, np.uint8), metric) == R.NONE).all()
        assert (R.distance_transform(np.full((6, 7), 1, np.uint8), metric) == INF).all()
        img = np.full((6, 2), 9, np.uint8)
        img[:, 0] = 0
        assert _all_ways(img, metric).tolist() == [[0, 1]] * 6
    assert (R.distance_transform(np.full((6, 7), 255, np.uint8), R.L1, np.uint8) == 255).all()
    far = np.full((1, 300), 255, np.uint8)
    far[0, 0] = 0
    got = R.distance_transform(far, R.L1, np.uint8)
    assert got[0, 254] == 254 and got[0, 255] == 255 and got[0, 299] == 255
    assert R.distance_transform(far, R.L1)[0, 299] == 299


def test_the_root_is_taken_of_the_float32_of_the_square():
    """above 2^24 the integer is rounded to float32 first, as the sum of two exact float32 squares is"""
    d2 = np.array([[4095 * 4095 + 4094 * 4094]], np.int64)
    assert d2[0, 0] > 1 << 24 and np.float32(d2[0, 0]) != d2[0, 0]
    assert R.finish(d2, R.L2).tobytes() == np.sqrt(np.float32(4095 * 4095) + np.float32(4094 * 4094)).tobytes()


def test_min_max_loc_ties_masks_nan_and_infinities():
    a = np.array([[5, 1, 9, 1], [9, 5, 1, 9]], np.uint8)
    assert R.min_max_loc(a) == (1.0, 9.0, (1, 0), (2, 0))
    m = np.array([[1, 0, 0, 255], [1, 1, 1, 1]], np.uint8)
    assert R.min_max_loc(a, m) == (1.0, 9.0, (3, 0), (0, 1))
    assert R.min_max_loc(a, np.zeros_like(a)) == (0.0, 0.0, (-1, -1), (-1, -1))
    f = np.array([[np.nan, 2.0, -np.inf], [np.inf, np.nan, np.inf]], np.float32)
    assert R.min_max_loc(f) == (-np.inf, np.inf, (2, 0), (0, 1))
    assert R.min_max_loc(np.full((2, 2), np.nan, np.float32)) == (0.0, 0.0, (-1, -1), (-1, -1))
    z = np.array([[0.0, -0.0], [-0.0, 0.0]], np.float32)
    assert R.min_max_loc(z)[2:] == ((0, 0), (0, 0))
    disc = np.zeros((64, 64), np.uint8)
    yy, xx = np.indices(disc.shape)
    disc[(yy - 31) ** 2 + (xx - 33) ** 2 <= 400] = 255
    # the nearest pixel outside dx^2 + dy^2 <= 400 is at (20, 1): 401
    assert R.largest_inscribed_circle(disc) == ((33, 31), float(np.sqrt(np.float32(401))))
