"""CPU suite of the statement of robust plane fitting (tests/plane_restate.py), on its own: it recovers the
generating plane of every synthetic case of tests/plane_cases.py and finds all generated inliers at four noise sigmas; the
orientation rule and the void rules hold; the sampler and the stop table are the motion model's; and the refit tolerance of
plane_cases.py is what the statement's own three summation orders give."""
import math

import numpy as np
import pytest

import model_restate as M
import plane_cases as K
import plane_restate as R

TRUTH = [c for c in K.CASES if c.truth is not None]


@pytest.mark.parametrize("case", TRUTH, ids=[c.id for c in TRUTH])
def test_statement_recovers_the_generating_plane(case):
    w = K.stated(case.id)
    assert w["found"] and case.threshold == 4 * K.SIGMA
    _, idx = R.points_of(case.xyz, case.box, case.mask)
    cand = np.zeros(case.h * case.w, bool)
    cand[idx] = True
    good = case.good.reshape(-1) & cand
    assert good.sum() >= 3 and (w["inliers"].reshape(-1)[good] == 255).all(), "a generated inlier is missing"
    assert w["n_inliers"] == int((w["inliers"] == 255).sum()) and not (w["inliers"].reshape(-1)[~cand]).any()
    for plane in (w["result"][0:4], w["result"][4:8]):
        assert K.angle(plane[:3], case.truth[:3]) < 0.02 and abs(plane[3] - case.truth[3]) < 0.02
        assert plane[3] > 0 and abs(np.linalg.norm(plane[:3]) - 1) < 1e-12
    assert w["result"][11] < 2 * case.threshold


def test_cases_without_a_model_and_the_search_lengths():
    for c in K.CASES:
        w = K.stated(c.id)
        assert w["found"] == c.found, c.id
        if not c.found:
            assert w["best_j"] == -1 and w["n_inliers"] == 0 and not w["inliers"].any() and not any(w["result"]), c.id
    assert [K.stated(i)["n_usable"] for i in ("two_points", "none_zeros", "none_nan", "none_inf")] == [2, 0, 0, 0]
    assert [K.stated(i)["n_hypotheses"] for i in ("two_points", "none_zeros")] == [0, 0], "fewer than three points: nothing is searched"
    for cid in ("through_origin", "along_z_vertical_wall"):
        w = K.stated(cid)
        assert w["void"] == w["n_hypotheses"] == K.BY_ID[cid].max_iters, "every hypothesis is void"
    assert K.stated("perp_vertical_wall")["found"] and K.stated("perp_vertical_wall")["n_inliers"] == 60
    w = K.stated("outliers_50_stops_early")
    assert w["n_hypotheses"] % R.ROUND == 0 and w["n_hypotheses"] < 2000
    assert K.stated("outliers_90_cut_at_44")["n_hypotheses"] == 300 == R.ROUND + 44
    assert K.stated("five_hypotheses")["n_hypotheses"] == 5
    assert K.stated("three_points")["n_inliers"] == 3
    w = K.stated("collinear_plus_one")
    assert w["found"] and w["n_inliers"] == 4 and w["void"] > 0
    assert K.stated("two_planes_60_40")["n_inliers"] == 720
    assert K.stated("slant_45_perp")["n_inliers"] != K.stated("slant_45_along_z")["n_inliers"]
    usable = sorted(K.stated(c.id)["n_usable"] for c in K.CASES if c.id.startswith("usable_"))
    _, g = K.geometry()
    assert usable == sorted(s + d for s in {64, int(g[0]), int(g[1])} for d in (-1, 0, 1))


def test_ties_go_to_the_lowest_index():
    c = K.BY_ID["set_twice"]
    w = K.stated(c.id)
    pts, _ = R.points_of(c.xyz)
    ties = [j for j in range(w["n_hypotheses"])
            if (lambda P: P is not None and int(R.inliers(P, c.metric, pts, c.threshold).sum()) == w["n_inliers"])(R.hypothesis(pts, c.metric, c.seed, j)[1])]
    assert w["n_inliers"] % 2 == 0 and ties[0] == w["best_j"]


def test_orientation_and_void_rules():
    p0, p1, p2 = [0.0, 0.0, 2.0], [1.0, 0.0, 2.0], [0.0, 1.0, 2.0]
    for a, b, c in ((p0, p1, p2), (p0, p2, p1)):                       # both windings: the same plane, towards the camera
        assert R.plane_from(a, b, c, R.PERP) == [0.0, 0.0, -1.0, 2.0]
    assert R.plane_from(p0, p1, [0.0, 1.0, -2.0], R.PERP)[3] > 0
    assert R.plane_from(p0, p0, p2, R.PERP) is None and R.plane_from(p0, p1, p1, R.PERP) is None, "equal points"
    assert R.plane_from(p0, p1, [2.0, 0.0, 2.0], R.PERP) is None, "collinear"
    assert R.plane_from(p0, p1, [2.0, 5e-7, 2.0], R.PERP) is None and R.plane_from(p0, p1, [2.0, 5e-6, 2.0], R.PERP) is not None, "the sine bound of 1e-6"
    assert R.plane_from([1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0, -1.0, 0.0], R.PERP) is None, "through the origin: d == 0"
    assert R.plane_from([1e200, 0.0, 1.0], [0.0, 1e200, 1.0], [0.0, 0.0, 1.0], R.PERP) is None, "not finite"
    wall = ([1.0, 0.0, 1.0], [1.0, 1.0, 2.0], [1.0, -1.0, 3.0])
    assert R.plane_from(*wall, R.PERP) == [-1.0, 0.0, 0.0, 1.0] and R.plane_from(*wall, R.ALONG_Z) is None
    steep = ([1.0, 0.0, 1.0], [1.0, 1.0, 2.0], [1.0 + 5e-7, -1.0, 3.0])
    assert R.plane_from(*steep, R.PERP) is not None and R.plane_from(*steep, R.ALONG_Z) is None, "|n2| <= 1e-6"


def test_sampler_and_stop_table_are_the_models():
    assert R.sample is M.sample and R.stop_table is M.stop_table and R.ROUND == M.ROUND == 256
    pts = np.arange(30, dtype=np.float32).reshape(10, 3)
    for j in range(40):
        s, _ = R.hypothesis(pts, R.PERP, 7, j)
        assert s == M.sample(10, 3, 7, j)[0][:3]
    lib = K.library()
    for n, conf, iters in ((3, 0.99, 300), (100, 0.99, 2000), (1025, 0.999, 65536), (600, 0.5, 700)):
        need, rounds = np.zeros(256, np.int32), np.zeros(1, np.int32)
        assert lib.vp_model_stop_table(n, M.AFFINE, conf, iters, need.ctypes.data, 256, rounds.ctypes.data) == 0
        assert need[:rounds[0]].tolist() == R.stop_table(n, M.AFFINE, conf, iters)


def test_refit_tolerance_is_measured_on_the_statement():
    spread = np.zeros(4)
    for c in K.CASES:
        if not K.stated(c.id)["found"]:
            continue
        three = [K.stated(c.id, order)["result"] for order in ("index", "reversed", "pairwise")]
        for a in range(3):
            for b in range(a + 1, 3):
                spread = np.maximum(spread, K.refit_differences(three[a], three[b]))
    print("refit spreads (angle, d, centroid, rms):", [repr(float(v)) for v in spread])
    assert spread.tolist() == pytest.approx([K.SPREAD_ANGLE, K.SPREAD_D, K.SPREAD_CENTROID, K.SPREAD_RMS], rel=1e-6, abs=0)
    assert (K.TOL_ANGLE, K.TOL_D, K.TOL_CENTROID, K.TOL_RMS) == tuple(64 * v for v in (K.SPREAD_ANGLE, K.SPREAD_D, K.SPREAD_CENTROID, K.SPREAD_RMS))


def test_refit_alone():
    c = K.BY_ID["two_planes_60_40"]
    pts, _ = R.points_of(c.xyz)
    keep = c.good.reshape(-1)
    for metric in (R.PERP, R.ALONG_Z):
        r = R.refit(pts, keep, metric)
        assert K.angle(r[:3], c.truth[:3]) < 2e-3 and abs(r[3] - c.truth[3]) < 2e-3 and r[4:8] == [0.0] * 4 and r[11] < 2 * K.SIGMA
        assert np.allclose(r[8:11], pts[keep].astype(np.float64).mean(0), atol=1e-12)
    line = np.array([[0, 0, 1], [1, 1, 2], [2, 2, 3], [3, 3, 4]], np.float32)
    assert R.refit(line, None, R.PERP) is None and R.refit(line, None, R.ALONG_Z) is None and R.refit(line[:2], None, R.PERP) is None
