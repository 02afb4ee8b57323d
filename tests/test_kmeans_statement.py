"""The statement of the colour k-means (tests/kmeans_restate.py) against answers worked out by hand: what the
GPU suite compares libvp with must itself say what the contract says."""
import numpy as np

import kmeans_restate as R


def _two_colours():
    img = np.zeros((6, 8, 3), np.uint8)
    img[:, :5] = (10, 20, 30)
    img[:, 5:] = (200, 100, 50)
    return img


def test_two_colours_converge_to_exactly_those_colours():
    """pass 1 assigns with the centres started elsewhere; update 1 lands on the two colours (shift > eps^2: not converged); pass 2
    assigns the same way; update 2 moves nothing (shift 0 <= eps^2: converged); pass 3 is the one more assign: 3 passes"""
    img = _two_colours()
    r = R.run(img, [[0, 0, 0], [255, 128, 0]], 10, 1.0)        # (200, 100, 50) is 6309 from the second centre, 52500 from the first
    assert r["iterations"] == 3
    assert r["centers"].dtype == np.float32 and r["centers"].tolist() == [[10, 20, 30], [200, 100, 50]]
    assert r["compactness"] == 0.0
    assert r["counts"].tolist() == [30, 18] and r["counts"].dtype == np.uint32
    exp = np.zeros((6, 8), np.int32)
    exp[:, 5:] = 1
    assert r["labels"].dtype == np.int32 and np.array_equal(r["labels"], exp)
    assert r["s1"].tolist() == [[300, 600, 900], [3600, 1800, 900]]
    assert r["s2"].dtype == np.uint64 and r["s2"].tolist() == [[3000, 12000, 27000], [720000, 180000, 45000]]


def test_a_tie_goes_to_the_lower_index():
    img = np.full((1, 4), 10, np.uint8)
    lab, n, s1, s2 = R.assign(R.samples(img), np.array([[5], [15]], np.float32))
    assert lab.tolist() == [0, 0, 0, 0] and n.tolist() == [4, 0]
    lab, *_ = R.assign(R.samples(img), np.array([[15], [5]], np.float32))
    assert lab.tolist() == [0, 0, 0, 0]
    lab, *_ = R.assign(R.samples(img), np.array([[16], [5], [15]], np.float32))
    assert lab.tolist() == [1, 1, 1, 1]


def test_an_empty_cluster_keeps_its_centre_and_counts_zero():
    img = np.array([[0, 0, 2, 2]], np.uint8)
    r = R.run(img, [[1.0], [200.5]], 5, 0.0)
    assert r["centers"].tolist() == [[1.0], [200.5]] and r["counts"].tolist() == [4, 0]
    assert r["labels"].tolist() == [[0, 0, 0, 0]]
    assert r["compactness"] == 4.0                      # four pixels at distance 1 from the centre 1.0
    assert r["iterations"] == 2                         # update 1 moves nothing: converged, one more pass


def test_one_pass_returns_the_initial_centres_with_their_labels():
    img = _two_colours()
    c0 = np.array([[0, 0, 0], [255, 255, 255]], np.float32)
    r = R.run(img, c0, 1, 0.0)
    assert r["iterations"] == 1 and r["centers"].tobytes() == c0.tobytes()
    # (10, 20, 30) is nearer to black, (200, 100, 50) too: 52500 against 69075
    assert r["labels"].tolist() == np.zeros((6, 8), int).tolist() and r["counts"].tolist() == [48, 0]
    d0, d1 = 30 * (100 + 400 + 900), 18 * (40000 + 10000 + 2500)
    assert r["compactness"] == float(d0 + d1)


def test_a_large_epsilon_stops_after_the_second_assign():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    r = R.run(img, [[0, 0, 0], [255, 255, 255], [128, 0, 255]], 50, 1000.0)
    assert r["iterations"] == 2
    px = R.samples(img)
    lab, n, s1, _ = R.assign(px, np.array([[0, 0, 0], [255, 255, 255], [128, 0, 255]], np.float32))
    assert r["centers"].tobytes() == R.update(np.array([[0, 0, 0], [255, 255, 255], [128, 0, 255]], np.float32), n, s1).tobytes()
    assert np.array_equal(r["labels"].ravel(), R.assign(px, r["centers"])[0])


def test_update_rounds_once_to_double_and_once_to_float32():
    n = np.array([3, 7], np.uint32)
    s1 = np.array([[10], [100]], np.uint32)
    c = R.update(np.zeros((2, 1), np.float32), n, s1)
    assert c.dtype == np.float32 and c[0, 0] == np.float32(10.0 / 3.0) and c[1, 0] == np.float32(100.0 / 7.0)
    assert R.shift(np.array([[3.0, 4.0], [1.0, 0.0]], np.float32), np.zeros((2, 2), np.float32)) == 25.0


def test_the_compactness_formula_agrees_with_the_direct_sum():
    """relative 1e-9: the cancellation in S2 - 2 c S1 + n c^2 costs about N 65025 2^-52 against a sum of order N 10^3"""
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    px = R.samples(img)
    r = R.run(img, R.seeded(img, [5, 900, 2000, 4000]), 6, 0.0)
    c = r["centers"].astype(np.float64)
    direct = np.sum((px.astype(np.float64) - c[r["labels"].ravel()]) ** 2)
    assert abs(r["compactness"] - direct) <= 1e-9 * direct
    assert r["counts"].sum() == 64 * 64 and int(r["s1"].sum()) == int(px.astype(np.int64).sum())
