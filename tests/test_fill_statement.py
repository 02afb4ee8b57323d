"""The integer crossings libvp fills polygons with (tests/fill_restate.py spans_restate) give the spans of the float64 scanline
`vision.utils.draw._fill`, for coordinates up to +-32767.  Host arithmetic only: runs without a GPU."""
import numpy as np
import pytest

import fill_restate as R


def test_cases_have_the_spans_of_fill():
    for name, polys in R.CASES.items():
        for p in polys:
            for h, w in ((110, 200), (110, 64), (40, 65)):
                assert R.spans_restate(p, h, w) == R.spans_of_fill(p, h, w), (name, h, w)


@pytest.mark.parametrize("seed", range(4))
def test_random_polygons_up_to_the_bound(seed):
    """Vertices anywhere in +-32767 on both axes, so that the denominators and the products are as large as they get; the image
    clips the rows to a band (the row loop is Python) and is wide enough to keep the right half of the spans."""
    rng = np.random.default_rng(seed)
    checked = 0
    for k in range(60):
        n = int(rng.integers(3, 9))
        pts = rng.integers(-R.MAX_COORD, R.MAX_COORD + 1, (n, 2))
        if k % 3 == 0:
            pts[rng.integers(0, n)] = rng.choice([-R.MAX_COORD, R.MAX_COORD], 2)     # a corner of the range
        if k % 4 == 1:
            pts[:, 1] = rng.integers(-3, 40, n)                                       # many vertices on the rows that are visited
        got, want = R.spans_restate(pts, 36, 40000), R.spans_of_fill(pts, 36, 40000)
        assert got == want, (seed, k, pts.tolist())
        checked += len(want)
    assert checked > 200


def test_small_dense_polygons():
    """Small coordinates: every row is visited, crossings at integers, halves and thirds, shared vertices, repeated points."""
    rng = np.random.default_rng(11)
    for k in range(150):
        n = int(rng.integers(1, 10))
        pts = rng.integers(-6, 30, (n, 2))
        if k % 5 == 0 and n > 2:
            pts[1] = pts[0]
        assert R.spans_restate(pts, 24, 24) == R.spans_of_fill(pts, 24, 24), pts.tolist()


def test_keys_order_as_the_rationals():
    """Two crossings with the largest denominators that differ by the least possible amount still get different, ordered keys; equal
    rationals with different denominators get equal keys."""
    a = R.cross_key(0, 0, 1, 65534, 1)              # 1 / 65534
    b = R.cross_key(0, 0, 1, 65533, 1)              # 1 / 65533
    assert a < b
    assert R.cross_key(0, 0, 2, 4, 1) == R.cross_key(0, 0, 3, 6, 1) == (32768 << 32) | (1 << 31)
    assert R.cross_key(5, 0, -5, 4, 1) == ((32768 + 2) << 32) | (1 << 31)            # 5 - 10 / 4 = 2.5
    assert R.cross_key(-5, 7, 5, 3, 4) == ((32768 + 2) << 32) | (1 << 31)            # upward edge: -5 + (-3)(10) / (-4) = 2.5
