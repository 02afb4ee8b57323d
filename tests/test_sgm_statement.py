"""CPU suite for the statement of semi-global matching: vp_stereo_sgm_host (scalar C++) equals tests/sgm_restate.py byte for byte on
every small case of tests/sgm_cases.py; the statement reduces to the pinned block matcher when the penalties are 0; a recurrence worked
out by hand; and the two properties the feature exists for - it answers a flat rectangle the block matcher leaves empty, and the
left-right check only ever removes pixels."""
import numpy as np
import pytest

import sgm_cases as SC
import sgm_restate as G
import stereo_restate as R
from stereo_cases import shifted_pair, two_plane_pair

CASES = SC.cases(SC.lib_plan)
SMALL = [c for c in CASES if c["oracle"] == "statement"]


@pytest.mark.parametrize("case", SMALL, ids=[c["id"] for c in SMALL])
def test_host_routine_equals_the_statement(case):
    left, right = case["pair"]()
    want = SC.expected(case)
    got = SC.host_disparity(left, right, **case["params"])
    assert got.dtype == np.int16 and np.array_equal(got, want), f"{int((got != want).sum())} pixels differ"


def test_cases_are_small_and_cover_what_they_claim():
    ids = {c["id"]: c for c in CASES}
    assert len(ids) == len(CASES)
    for c in SMALL:
        h, w = c["pair"]()[0].shape
        n = c["params"]["num_disparities"]
        assert h <= 48 and (w <= n + 80 or c["id"].startswith(("lr_", "min_-128", "min_128"))), c["id"]
    one = SC.expected(ids["tiny_one_pixel"])
    assert (one != -16).sum() == 1 and one[2, 17] != -16
    assert np.all(SC.expected(ids["tiny_empty_w"]) == -16) and np.all(SC.expected(ids["tiny_empty_h"]) == -16)
    assert SC.lib_plan(40, 5, 16, 5, 0)["rect"][3] == 1 and SC.lib_plan(20, 12, 16, 5, 0)["rect"][2] == 1
    for paths in (4, 8):        # a signed 16-bit sum would show: the statement's own S passes 32767 and stays within 65535
        c = ids[f"penalty_largest_p{paths}"]
        p = G.resolve(c["params"])
        assert G.admitted(p) and not G.admitted({**p, "p2": p["p2"] + 1})
        S = G.summed_costs(*c["pair"](), **c["params"])[0]
        assert 32767 < S.max() <= 65535
    flat = SC.expected(ids["flat_ties"])
    x, y, cw, ch = R.valid_rect(70, 24, 32, 5, 0)
    assert np.all(flat[y:y + ch, x:x + cw] == 31 * 16) and np.all(SC.expected(ids["flat_unique"]) == -16)      # ties to the larger d everywhere
    assert np.any(SC.expected(ids["uniq_100"]) != SC.expected(ids["uniq_0"])) and np.any(SC.expected(ids["uniq_15"]) != SC.expected(ids["uniq_0"]))
    for m in (0, 2):
        counts = [int((SC.expected(ids[f"lr_m{m}_d{d}"]) != (m - 1) * 16).sum()) for d in (0, 1, 255, -1)]
        assert counts[0] < counts[1] < counts[2] == counts[3]
    # the geometry cases sit on the block boundaries the plan reports
    for n in (16, 32, 64):
        p = SC.lib_plan(200 + n, 40, n, 5, 0)
        lpb, ppb = p["path"]["lines_per_block"], p["select"]["px_per_block"]
        assert lpb == 64 // p["path"]["group"] and ppb == 256 // p["path"]["group"]
        rects = SC.geometry_rects(SC.lib_plan, n)
        for v in (lpb, lpb + 1):
            for pick in (lambda cw, ch: ch, lambda cw, ch: cw, lambda cw, ch: cw + ch - 1):
                assert any(pick(cw, ch) == v for cw, ch in rects), (n, v)
        for cw, ch in rects:
            h, w = SC.size_for(cw, ch, n, 5)
            q = SC.lib_plan(w, h, n, 5, 0)
            assert q["rect"][2:] == (cw, ch)
            assert q["path"]["grid_h"] == -(-ch // lpb) and q["path"]["grid_v"] == -(-cw // lpb) and q["path"]["grid_d"] == -(-(cw + ch - 1) // lpb)
            assert q["select"]["grid"] == -(-(cw * ch) // ppb)
        assert {cw * ch for cw, ch in rects} >= {ppb - 1, ppb, ppb + 1}
    strip = SC.lib_plan(200, 40, 16, 5, 0)["cost"]["strip_cols"]
    assert [SC.lib_plan(SC.size_for(cw, 3, 16, 5)[1], 7, 16, 5, 0)["cost"]["grid"] for cw in (strip - 1, strip, strip + 1, 2 * strip + 1)] == [(1, 3), (1, 3), (2, 3), (3, 3)]
    assert [SC.lib_plan(200, 40, n, 5, 0)["path"]["per_lane"] for n in (16, 64, 80, 128, 144, 256)] == [1, 1, 2, 2, 4, 4]


@pytest.mark.parametrize("paths", (4, 8))
@pytest.mark.parametrize("block_size", (5, 7, 9))
def test_without_penalties_it_is_the_block_matcher(block_size, paths):
    """S is then paths * C, the argmin and the uniqueness-free selection are the block matcher's and the subpixel quotient is scale-free"""
    left, right = shifted_pair(30, 100, 5, 3, noise=20)
    p = dict(num_disparities=16, block_size=block_size, p1=0, p2=0, uniqueness_ratio=0, disp12_max_diff=-1, paths=paths)
    want = R.disparity(left, right, num_disparities=16, block_size=block_size, texture_threshold=0, uniqueness_ratio=0)
    assert np.any(want != -16)
    assert np.array_equal(G.disparity(left, right, **p), want)
    assert np.array_equal(SC.host_disparity(left, right, **p), want)


def test_a_recurrence_worked_out_by_hand():
    """a 1 x 3 candidate row, n = 16, p1 = 4, p2 = 15; every entry of C is 50 but the ones named"""
    C = np.full((1, 3, 16), 50, np.int64)
    C[0, 0, 3], C[0, 0, 4] = 2, 10
    C[0, 1, 4], C[0, 1, 9] = 1, 0
    C[0, 2, 0], C[0, 2, 5], C[0, 2, 15] = 7, 3, 20
    # (0, 1): L0 = C0, M = 2, so M + p2 = 17; then M = 5 and M + p2 = 20
    right = np.array([C[0, 0],
                      [65, 65, 54, 50, 5, 62, 65, 65, 65, 15, 65, 65, 65, 65, 65, 65],
                      [22, 65, 65, 54, 50, 7, 65, 65, 64, 60, 64, 65, 65, 65, 65, 35]])
    # (0, -1): L2 = C2, M = 3, M + p2 = 18; then M = 5
    left = np.array([[65, 65, 65, 6, 10, 54, 65, 65, 64, 60, 64, 65, 65, 65, 65, 65],
                     [54, 58, 65, 65, 5, 50, 54, 65, 65, 15, 65, 65, 65, 65, 65, 65],
                     C[0, 2]])
    assert np.array_equal(G.path_costs(C, 0, 1, 4, 15)[0], right)
    assert np.array_equal(G.path_costs(C, 0, -1, 4, 15)[0], left)
    # a single row: a vertical or diagonal step has no predecessor
    for dy, dx in G.DIRECTIONS[2:]:
        assert np.array_equal(G.path_costs(C, dy, dx, 4, 15), C)


@pytest.mark.parametrize("disp12_max_diff", (-1, 1))
@pytest.mark.parametrize("paths", (4, 8))
def test_a_flat_rectangle_is_answered_where_the_block_matcher_is_not(paths, disp12_max_diff):
    """Two conditions, not measurements: the block matcher leaves all of the rectangle's interior invalid, semi-global matching answers
    all of it within one disparity of the truth, 6.  (The shares measured on the CPU: 1.0 and 1.0, in all four settings.)"""
    left, right = (a.copy() for a in shifted_pair(40, 160, 6, 7))
    left[10:30, 70:110] = 128
    right[10:30, 64:104] = 128
    bm = R.disparity(left, right, num_disparities=16, block_size=5)
    assert np.all(bm[13:27, 73:107] == -16)
    p = dict(num_disparities=16, block_size=5, p1=8, p2=32, uniqueness_ratio=10, paths=paths, disp12_max_diff=disp12_max_diff)
    got = G.disparity(left, right, **p)
    assert np.all(np.abs(got[13:27, 73:107].astype(np.int32) - 96) <= 16)
    assert np.array_equal(SC.host_disparity(left, right, **p), got)


def test_the_left_right_check_only_removes():
    left, right = two_plane_pair(40, 160, 7)
    p = dict(num_disparities=16, block_size=5, p1=8, p2=32, uniqueness_ratio=0)
    free, checked = G.disparity(left, right, **p, disp12_max_diff=-1), G.disparity(left, right, **p, disp12_max_diff=1)
    removed = (free != -16) & (checked == -16)
    assert removed.sum() > 0
    assert np.array_equal(checked[~removed], free[~removed])
