"""CPU suite of the statement of the features over a scale pyramid (tests/pyr_features_restate.py): the
level-size rule on hand-checked sizes, the quotas, and the three recognition scenes on which the statement alone must find the
source - at half its size, at its own size turned by 10 degrees, and at twice its size - with the corner errors the bound of
tests/test_gpu_pyr_features.py is taken from."""
import numpy as np

import features_cases as K
import pyr_features_cases as PC
import pyr_features_restate as P


def test_level_sizes_on_hand_checked_sides():
    assert P.level_sizes(37, 37, 8) == [(37, 37), (31, 31)]            # (5 * 37 + 3) // 6 = 31, then 26
    assert P.level_sizes(36, 36, 8) == [(36, 36)]                      # (5 * 36 + 3) // 6 = 30
    assert P.level_sizes(30, 30, 8) == [] and P.level_sizes(30, 400, 8) == [] and P.level_sizes(400, 30, 3) == []
    assert P.level_sizes(1920, 1080, 8) == [(1920, 1080), (1600, 900), (1333, 750), (1111, 625), (926, 521), (772, 434), (643, 362), (536, 302)]
    assert P.level_sizes(1920, 1080, 3) == [(1920, 1080), (1600, 900), (1333, 750)] and P.level_sizes(1920, 1080, 1) == [(1920, 1080)]
    assert P.level_sizes(37, 200, 8) == [(37, 200), (31, 167)], "the smaller side decides"


def test_quotas_sum_to_the_budget_and_level_zero_takes_the_rest():
    sizes = P.level_sizes(1920, 1080, 8)
    areas = [w * h for w, h in sizes]
    for n in (0, 1, 7, 500, 2000, 10000, 1 << 20):
        q = P.quotas(sizes, n)
        assert sum(q) == n and all(v >= 0 for v in q)
        assert q[1:] == [n * a // sum(areas) for a in areas[1:]] and q[0] == n - sum(q[1:]) and q[0] >= n * areas[0] // sum(areas)
    assert P.quotas(sizes, 1) == [1, 0, 0, 0, 0, 0, 0, 0] and P.quotas([], 5) == []
    assert P.quotas([(37, 37), (31, 31)], 100) == [59, 41]             # 100 * 961 // 2330 = 41
    assert P.quotas(P.level_sizes(131, 97, 8), 3) == [3, 0, 0, 0, 0, 0, 0]


def test_the_statement_states_what_it_says():
    img = PC.soft_noise(97, 131, 5)
    pts0, desc, lev, score, bins, lxy = P.pyramid_features(img, 5, 400)
    sizes = P.level_sizes(131, 97, 8)
    q = P.quotas(sizes, 400)
    assert len(pts0) <= 400 and [int((lev == l).sum()) <= q[l] for l in range(len(sizes))] == [True] * len(sizes)
    order = np.lexsort((lxy[:, 1], lxy[:, 2], lxy[:, 0]))
    assert np.array_equal(order, np.arange(len(lxy))), "level, then y, then x"
    for l, (w, h) in enumerate(sizes):
        at = lxy[lev == l]
        assert (at[:, 1] >= 15).all() and (at[:, 1] <= w - 16).all() and (at[:, 2] >= 15).all() and (at[:, 2] <= h - 16).all()
    assert np.array_equal(pts0[lev == 0], lxy[lev == 0][:, 1:].astype(np.float32)), "level 0 reports its own pixels"
    x = lxy[lev == 1][:, 1]
    assert np.array_equal(pts0[lev == 1][:, 0], ((x + 0.5) * (131 / 109) - 0.5).astype(np.float32))
    assert float(P.keypoint_size(131, 109)) == float(np.float32(31.0 * 131 / 109))
    assert len(P.pyramid_features(np.zeros((30, 40), np.uint8), 5, 100)[0]) == 0 and len(P.pyramid_features(img, 5, 0)[0]) == 0
    one = P.pyramid_features(img, 5, 400, levels=1)
    assert (one[2] == 0).all() and len(one[0]) == 400


def test_the_statement_alone_finds_the_source_at_all_three_scales():
    figures = {}
    for which in PC.SCALES:
        out = PC.stated_recognition(which)
        assert out["H"] is not None and len(out["q"]) >= K.MIN_MATCH and out["inliers"] >= K.MIN_MATCH, which
        figures[which] = out["corner_error"]
        print(which, "corner error", out["corner_error"], "good", len(out["q"]), "inliers", out["inliers"])
        assert abs(out["corner_error"] - PC.CORNER_ERROR_MEASURED[which]) < 1e-6, (which, out["corner_error"])
    assert PC.CORNER_ERROR_BOUND == 2 * max(PC.CORNER_ERROR_MEASURED.values()) and PC.CORNER_ERROR_BOUND <= K.RANSAC_THRESHOLD
    assert (PC.TEX_W, PC.TEX_H) == (192, 160) and PC.scene("half")[0].shape == (200, 240) and PC.scene("double")[0].shape == (260, 320)
