"""CPU suite of the statement of robust rigid motion (tests/rigid_restate.py), on its own: it recovers the
generating motion of every synthetic case of tests/rigid_cases.py within the bounds measured there, never admits a gross outlier
and never proposes a reflection; the void rules, the search lengths, the tie rule and the two metrics hold; and the refit tolerance of
rigid_cases.py is what the statement's own three summation orders give."""
import numpy as np
import pytest

import model_restate as M
import rigid_cases as K
import rigid_restate as R

TRUTH = [c for c in K.CASES if c.truth is not None]


@pytest.mark.parametrize("case", TRUTH, ids=[c.id for c in TRUTH])
def test_statement_recovers_the_generating_motion(case):
    w = K.stated(case.id)
    assert w["found"] and case.threshold == 4 * case.sigma
    rec = K.recovery(w["result"], case.truth)
    print(case.id, "errors / sigma (refit angle, refit t, hypothesis angle, hypothesis t):", [v / case.sigma for v in rec])
    for got, ratio in zip(rec, (K.RECOVER_REFIT_ROT, K.RECOVER_REFIT_T, K.RECOVER_HYP_ROT, K.RECOVER_HYP_T)):
        assert got <= 2 * ratio * case.sigma
    if case.gross is not None:
        assert not w["inliers"][case.gross].any(), "a gross outlier (10 thresholds away at least) is an inlier"
    assert w["n_inliers"] == int(w["inliers"].sum()) >= 3 and w["result"][30] < case.threshold
    P, Q, idx = R.pairs_of(case.src, case.dst)
    assert np.allclose(w["result"][24:27], P[w["inliers"][idx] == 1].astype(np.float64).mean(0), atol=1e-12)


def test_the_recovery_bounds_are_the_measured_ones():
    rec = np.zeros(4)
    for c in TRUTH:
        rec = np.maximum(rec, np.array(K.recovery(K.stated(c.id)["result"], c.truth)) / c.sigma)
    print("largest errors / sigma:", [repr(float(v)) for v in rec])
    assert rec.tolist() == pytest.approx([K.RECOVER_REFIT_ROT, K.RECOVER_REFIT_T, K.RECOVER_HYP_ROT, K.RECOVER_HYP_T], rel=1e-6, abs=0)
    assert sorted(c.sigma for c in TRUTH if c.id.startswith("noise_sigma_")) == list(K.SIGMAS)


def test_the_ego_motion_bounds_are_the_measured_ones():
    """the synthetic rig of rigid_cases.ego_scene: what the statement itself leaves of the known motion, twice which is the bound"""
    s, w = K.ego_scene(), K.ego_stated()
    assert w["found"] and int(s["status"].sum()) > 200 and w["n_usable"] <= int(s["status"].sum()) and w["n_inliers"] > 0.8 * w["n_usable"]
    assert not w["inliers"][~s["status"]].any()
    ang, dt = K.recovery(w["result"], K.EGO_MOTION)[:2]
    print("ego scene: refit angle %r rad, |dt| %r m, %d of %d pairs" % (ang, dt, w["n_inliers"], w["n_usable"]))
    assert [ang, dt] == pytest.approx([K.EGO_MEASURED_ROT, K.EGO_MEASURED_T], rel=1e-6, abs=0)
    assert (K.EGO_BOUND_ROT, K.EGO_BOUND_T) == (2 * K.EGO_MEASURED_ROT, 2 * K.EGO_MEASURED_T)
    assert K.EGO_BOUND_ROT < 0.1 * K.rot_angle(K.EGO_MOTION[0], np.eye(3)) and K.EGO_BOUND_T < 0.1 * np.linalg.norm(K.EGO_MOTION[1]), "a small part of the motion"


def test_no_reflection_is_ever_proposed():
    for cid in ("usable_65", "mirrored", "near_far_euclid", "sources_collinear"):
        c = K.BY_ID[cid]
        P, Q, _ = R.pairs_of(c.src, c.dst)
        valid = 0
        for j in range(256):
            _, m = R.hypothesis(P, Q, c.seed, j)
            if m is None:
                continue
            valid += 1
            Rm = np.array(m[:9]).reshape(3, 3)
            assert abs(np.linalg.det(Rm) - 1.0) <= 1e-12 and np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-12
        assert (valid == 0) == (cid == "sources_collinear")


def test_cases_without_a_model_and_the_search_lengths():
    for c in K.CASES:
        w = K.stated(c.id)
        if c.found is not None:
            assert w["found"] == c.found, c.id
        if not w["found"]:
            assert w["best_j"] == -1 and w["n_inliers"] == 0 and not w["inliers"].any() and not any(w["result"]), c.id
    assert [K.stated(i)["n_usable"] for i in ("one_pair", "two_pairs", "none_zeros", "none_nan", "none_inf")] == [1, 2, 0, 0, 0]
    assert [K.stated(i)["n_hypotheses"] for i in ("two_pairs", "none_zeros")] == [0, 0], "fewer than three pairs: nothing is searched"
    for cid in ("sources_collinear", "destinations_collinear"):
        w = K.stated(cid)
        assert w["void"] == w["n_hypotheses"] == K.BY_ID[cid].max_iters == 300 and not w["found"], "every hypothesis is void"
    assert [K.stated(i)["n_hypotheses"] for i in ("five_hypotheses", "iters_256", "iters_257")] == [5, 256, 257]
    w = K.stated("outliers_90_cut_at_44")
    assert w["n_hypotheses"] == 300 == R.ROUND + 44 and w["found"] and w["best_j"] >= R.ROUND
    w = K.stated("outliers_50_stops_early")
    assert w["n_hypotheses"] % R.ROUND == 0 and w["n_hypotheses"] < 2000
    assert K.stated("three_pairs")["n_inliers"] == 3
    assert K.stated("two_motions_60_40")["n_inliers"] == 360, "the larger motion wins"


def test_ties_go_to_the_lowest_index():
    c = K.BY_ID["set_twice"]
    w = K.stated(c.id)
    P, Q, _ = R.pairs_of(c.src, c.dst)
    ties = []
    for j in range(w["n_hypotheses"]):
        m = R.hypothesis(P, Q, c.seed, j)[1]
        if m is not None and int(R.inliers(m, c.metric, P, Q, c.threshold).sum()) == w["n_inliers"]:
            ties.append(j)
    assert w["n_inliers"] % 2 == 0 and ties[0] == w["best_j"]


def test_the_two_metrics_differ_where_stereo_noise_grows():
    e, d = K.stated("near_far_euclid"), K.stated("near_far_disparity")
    c = K.BY_ID["near_far_euclid"]
    far = c.src[:, 2] > 4
    assert d["n_inliers"] == c.n and e["n_inliers"] < c.n, "a fixed number of centimetres throws away points far off"
    assert e["inliers"][~far].all() and not e["inliers"][far].all()
    z = K.stated("disparity_z_not_positive")
    cz = K.BY_ID["disparity_z_not_positive"]
    assert z["found"] and not z["inliers"][cz.dst[:, 2] <= 0].any() and not z["inliers"][cz.src[:, 2] <= 0].any() and (cz.dst[:, 2] <= 0).sum() > 20


def test_a_mirrored_set_holds_no_motion():
    w = K.stated("mirrored")
    print("mirrored: the best hypothesis holds", w["n_inliers"], "of", w["n_usable"])
    assert w["n_inliers"] == K.MIRROR_MEASURED and w["n_inliers"] <= K.MIRROR_CAP < w["n_usable"] // 2


def test_tracks_give_the_pairs_the_rules_say():
    for c in K.TRACK_CASES:
        t = c.tracks
        pair = (c.src != 0).any(1)
        assert not pair[[0, 1, 2, 4, 5, 7, 8, 9]].any() and pair[[3, 6, 10]].all(), c.id
        assert not pair[c.n // 2] and pair[c.n // 2 + 1] and pair[c.n // 2 + 2], "status 0; 2 and 0xFFFFFFFF count as set"
        assert np.array_equal(c.src[6], t["xyz0"][R.pixel(t["prev"][6, 1], t["h"]), 3]), "x = 2.5 is pixel 3"
    assert (R.pixel(-0.5, 33), R.pixel(-0.51, 33), R.pixel(32.49, 33), R.pixel(32.5, 33), R.pixel(2.5, 33), R.pixel(np.nan, 33)) == (0, None, 32, None, 3, None)


def test_sampler_and_stop_table_are_the_models():
    assert R.sample is M.sample and R.stop_table is M.stop_table and R.ROUND == M.ROUND == 256
    c = K.BY_ID["usable_63"]
    P, Q, _ = R.pairs_of(c.src, c.dst)
    for j in range(40):
        assert R.hypothesis(P, Q, 7, j)[0] == M.sample(len(P), 3, 7, j)[0][:3]


def test_refit_tolerance_is_measured_on_the_statement():
    spread = np.zeros(4)
    for c in K.CASES:
        if not K.stated(c.id)["found"]:
            continue
        three = [K.stated(c.id, order)["result"] for order in ("index", "reversed", "pairwise")]
        for a in range(3):
            for b in range(a + 1, 3):
                spread = np.maximum(spread, K.refit_differences(three[a], three[b]))
    print("refit spreads (rotation, t, centroid, rms):", [repr(float(v)) for v in spread])
    assert spread.tolist() == pytest.approx([K.SPREAD_ROT, K.SPREAD_T, K.SPREAD_CENTROID, K.SPREAD_RMS], rel=1e-6, abs=0)
    assert (K.TOL_ROT, K.TOL_T, K.TOL_CENTROID, K.TOL_RMS) == tuple(64 * v for v in (K.SPREAD_ROT, K.SPREAD_T, K.SPREAD_CENTROID, K.SPREAD_RMS))


def test_refit_alone():
    c = K.BY_ID["two_motions_60_40"]
    r = R.refit(c.src, c.dst, c.good)
    rec = K.recovery(r, c.truth)
    assert rec[0] <= 2 * K.RECOVER_REFIT_ROT * c.sigma and rec[1] <= 2 * K.RECOVER_REFIT_T * c.sigma and r[12:24] == [0.0] * 12
    assert r[30] < 2 * 3 ** 0.5 * c.sigma, "least squares: no more than the generating motion leaves, whose noise is at most 2 sqrt(3) sigma long"
    line = np.array([[0, 0, 1], [1, 1, 2], [2, 2, 3], [3, 3, 4]], np.float32)
    assert R.refit(line, line + 1) is None and R.refit(line[:2], line[:2]) is None, "inliers on a line: degenerate"
    sq = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1], [1, 1, 2]], np.float32)
    r = R.refit(sq, sq @ K.MOTION_2[0].T.astype(np.float32) + K.MOTION_2[1].astype(np.float32))
    assert K.rot_angle(r[0:9], K.MOTION_2[0]) < 1e-6 and np.linalg.norm(np.array(r[9:12]) - K.MOTION_2[1]) < 1e-6
