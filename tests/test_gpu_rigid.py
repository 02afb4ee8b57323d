"""GPU suite of robust rigid motion (libvp vp_rigid.hip): vp_fit_rigid_dev / _f32 and the track forms are
compared bit for bit - best hypothesis, its index, the three counts, the inlier bytes - with the host forms and the statement
tests/rigid_restate.py on every case of tests/rigid_cases.py, and the refit within the tolerance measured on the statement."""
import numpy as np
import pytest

import rigid_cases as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", K.CASES, ids=K.IDS)
def test_device_fit_is_the_statements(vp, case):
    want = K.stated(case.id)
    host = K.call_host(case)
    K.same_exact(host, want, case.id + " host")
    for name, got in (("dev", K.call_dev(vp, case)), ("f32", K.call_f32(vp.default_context().handle, case))):
        what = "%s %s" % (case.id, name)
        K.same_exact(got, want, what)            # the canary tail behind the n inlier bytes included
        assert np.array_equal(got["result"][12:24].view(np.uint64), host["result"][12:24].view(np.uint64)) and got["counts"] == host["counts"], what
        assert np.array_equal(got["inliers"], host["inliers"]) and set(np.unique(got["inliers"]).tolist()) <= {0, 1}, what
        K.same_refit(got, want, what)


def test_usable_counts_straddle_the_kernel_boundaries():
    _, g = K.geometry()
    run, stage = int(g[0]), int(g[1])
    usable = sorted(K.stated(c.id)["n_usable"] for c in K.CASES if c.id.startswith("usable_"))
    assert usable == sorted({63, 64, 65, run - 1, run, run + 1, stage - 1, stage, stage + 1, 2 * stage + 1})
    assert [K.stated(i)["n_usable"] for i in ("none_zeros", "two_pairs", "three_pairs")] == [0, 2, 3]


def test_no_inlier_bytes_wanted(vp):
    for cid in ("usable_1025", "tracks_33x17"):
        case, want = K.BY_ID[cid], K.stated(cid)
        for got in (K.call_dev(vp, case, want_inliers=False), K.call_f32(vp.default_context().handle, case, want_inliers=False)):
            K.same_exact(got, want, cid)
            K.same_refit(got, want, cid)


def test_calls_of_different_sizes_on_one_context_carry_nothing_over(vp):
    order = ["usable_2049", "two_pairs", "usable_65", "sources_collinear", "tracks_257x9", "outliers_90_cut_at_44", "three_pairs", "none_nan", "near_far_disparity",
             "usable_2049"]
    for cid in order:
        got = K.call_dev(vp, K.BY_ID[cid])
        K.same_exact(got, K.stated(cid), cid)
        K.same_refit(got, K.stated(cid), cid)


@pytest.mark.parametrize("case", K.TRACK_CASES, ids=[c.id for c in K.TRACK_CASES])
def test_inlier_bytes_land_on_the_track_rows(vp, case):
    got, want = K.call_dev(vp, case), K.stated(case.id)
    t = case.tracks
    pair = (case.src != 0).any(1)
    assert not got["inliers"][~pair].any(), "a track that gives no pair is an inlier"
    assert not pair[[0, 1, 2, 4, 5, 7, 8, 9]].any() and pair[[3, 6, 10]].all(), "status 0, NaN, -0.51, w - 0.5, h - 0.5, unknown points; -0.5 and 2.5 are inside"
    assert np.array_equal(case.src[6], t["xyz0"][K.R.pixel(t["prev"][6, 1], t["h"]), 3]), "x = 2.5 is pixel 3"
    assert np.array_equal(got["inliers"], want["inliers"]) and got["counts"][0] == int(pair.sum())
