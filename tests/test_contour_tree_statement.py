"""CPU: the two statements of cv2.findContours' RETR_CCOMP / RETR_TREE (contour_tree_restate.py) against each other, the contours
they order against the oracle's RETR_LIST, the hierarchy's invariants, and the facade's mode check."""
import numpy as np
import pytest

import contour_tree_restate as R
import frames as F

MODES = (R.RETR_CCOMP, R.RETR_TREE)


def known_shapes():
    yy, xx = np.mgrid[0:60, 0:80]
    r2 = (xx - 40) ** 2 + (yy - 30) ** 2
    ring = (r2 <= 25 ** 2) & (r2 >= 18 ** 2)
    out = {"ring": ring, "ring_in_ring": ring | ((r2 <= 12 ** 2) & (r2 >= 7 ** 2))}
    m = np.zeros((40, 60), bool)
    m[5:35, 5:55] = True
    m[10:30, 10:50] = False
    m[15:20, 15:20] = True
    m[15:25, 35:45] = True
    out["two_islands_in_one_hole"] = m
    m = np.zeros((20, 30), bool)
    m[0:15, 0:20] = True
    m[0:6, 5:10] = False                              # a notch open to the top edge: background that reaches the frame, not a hole
    m[8:12, 8:12] = False
    out["hole_touching_frame"] = m
    out["1xN"] = np.array([[1, 1, 0, 1, 0, 0, 1, 1, 1]], bool)
    out["Nx1"] = out["1xN"].T.copy()
    out["all_foreground"] = np.ones((7, 9), bool)
    out["empty"] = np.zeros((5, 6), bool)
    return {k: v.astype(np.uint8) * 255 for k, v in out.items()}


def concentric(h, w, period=2):
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.minimum(np.minimum(yy, h - 1 - yy), np.minimum(xx, w - 1 - xx))
    return ((d % period) == 0).astype(np.uint8) * 255


def thin_wall_mask(rng, h, w):
    m = np.zeros((h, w), np.uint8)
    m[:, :] = 255
    m[1:h - 1, 1:w - 1] = 0
    if h > 4 and w > 4:
        m[2:h - 2, 2:w - 2] = ((rng.random((h - 4, w - 4)) < 0.6) * 255).astype(np.uint8)
    return m


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def check_invariants(starts, holes, hier):
    n = len(hier)
    key = [int(y) * 100000 + int(x) for y, x in starts]
    for i in range(n):
        nx, pv, fc, par = (int(v) for v in hier[i])
        if par >= 0:
            assert key[par] < key[i] and par < i
        if fc >= 0:
            assert fc == i + 1 and hier[fc][3] == i
        if nx >= 0:
            assert hier[nx][1] == i and hier[nx][3] == par
        if pv >= 0:
            assert hier[pv][0] == i and hier[pv][3] == par
            assert key[pv] > key[i]                   # newest first


@pytest.mark.parametrize("name", sorted(known_shapes()))
def test_statements_agree_on_known_shapes(name):
    m = known_shapes()[name]
    for mode in MODES:
        a, b = R.raster_scan(m, mode), R.topological(m, mode)
        assert _same(a, b), (name, mode)
        check_invariants(*a)


def test_known_answers():
    s, h, hier = R.raster_scan(known_shapes()["ring_in_ring"], R.RETR_TREE)
    assert h.tolist() == [0, 1, 0, 1]                 # outer ring, its hole, inner ring, its hole: one chain
    assert hier.tolist() == [[-1, -1, 1, -1], [-1, -1, 2, 0], [-1, -1, 3, 1], [-1, -1, -1, 2]]
    s, h, hier = R.raster_scan(known_shapes()["ring_in_ring"], R.RETR_CCOMP)
    # both rings at the top level, the inner (newer) one first, each followed by its hole
    assert h.tolist() == [0, 1, 0, 1] and s[0][0] > s[2][0]
    assert hier.tolist() == [[2, -1, 1, -1], [-1, -1, -1, 0], [-1, 0, 3, -1], [-1, -1, -1, 2]]
    s, h, hier = R.raster_scan(known_shapes()["empty"], R.RETR_TREE)
    assert len(s) == 0 and hier.shape == (0, 4)


def test_statements_agree_on_random_and_thin_wall_masks():
    rng = np.random.default_rng(404)
    n = 0
    for trial in range(420):
        h, w = int(rng.integers(1, 24)), int(rng.integers(1, 30))
        m = F.random_mask(rng, h, w) if trial % 3 else thin_wall_mask(rng, h, w)
        for mode in MODES:
            a, b = R.raster_scan(m, mode), R.topological(m, mode)
            assert _same(a, b), (trial, mode)
            check_invariants(*a)
            n += 1
    m = concentric(60, 70)                            # nested 30 deep
    for mode in MODES:
        assert _same(R.raster_scan(m, mode), R.topological(m, mode))
    assert n >= 800


@pytest.mark.parametrize("method", [1, 2])
def test_contour_sets_equal_the_oracles_list(oracle, method):
    rng = np.random.default_rng(7 + method)
    masks = list(known_shapes().values()) + [F.random_mask(rng, 20, 31) for _ in range(20)] + [thin_wall_mask(rng, 16, 19)]
    for m in masks:
        lst, lh = oracle.find_contours(m, 1, method, with_holes=True)
        for mode in MODES:
            got, holes, _ = R.expected(m, mode, lst)
            assert len(got) == len(lst)
            # the same borders, point for point, only reordered; each starts where the statement says
            key = lambda c: c.tobytes()                                        # noqa: E731
            assert sorted(map(key, got)) == sorted(map(key, lst))
            starts, _, _ = R.raster_scan(m, mode)
            if method == 1:                               # (CHAIN_APPROX_SIMPLE may drop a start that lies on a straight run)
                assert all(tuple(c[0, 0]) == (int(x), int(y)) for c, (y, x) in zip(got, starts))
            order = {key(c): k for k, c in enumerate(lst)}
            assert [int(lh[order[key(c)]]) for c in got] == holes.tolist()


def test_facade_rejects_unknown_modes():
    from vision import cv2_facade
    m = np.zeros((4, 4), np.uint8)
    for mode in (4, -1, 7):
        with pytest.raises(cv2_facade.error):
            cv2_facade.findContours(m, mode, cv2_facade.CHAIN_APPROX_SIMPLE)
    assert (cv2_facade.RETR_CCOMP, cv2_facade.RETR_TREE) == (2, 3)
