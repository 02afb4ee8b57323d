"""GPU suite of robust plane fitting (libvp vp_plane.hip): vp_fit_plane_dev and vp_fit_plane_f32 are compared
bit for bit - best hypothesis, its index, the three counts, the inlier image - with vp_fit_plane_host and the statement
tests/plane_restate.py on every case of tests/plane_cases.py, and the refit within the tolerance measured on the statement."""
import numpy as np
import pytest

import plane_cases as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", K.CASES, ids=K.IDS)
def test_device_fit_is_the_statements(vp, case):
    want = K.stated(case.id)
    host = K.call_host(case)
    K.same_exact(host, want, case.id + " host")
    for name, got in (("dev", K.call_dev(vp, case)), ("f32", K.call_f32(vp.default_context().handle, case))):
        K.same_exact(got, want, "%s %s" % (case.id, name))
        assert np.array_equal(got["result"][4:8].view(np.uint64), host["result"][4:8].view(np.uint64)) and got["counts"] == host["counts"]
        assert np.array_equal(got["inliers"], host["inliers"])
        K.same_refit(got, want, "%s %s" % (case.id, name))
        # the void share is the statement's: every hypothesis taken was formed and counted alike, or the best index and count would differ
        assert got["counts"][2] == want["n_hypotheses"]
        inl = got["inliers"]
        assert set(np.unique(inl).tolist()) <= {0, 255}
        if case.box is not None:
            x0, y0, rw, rh = case.box
            outside = np.ones((case.h, case.w), bool)
            outside[y0:y0 + rh, x0:x0 + rw] = False
            assert not inl[outside].any(), "a pixel outside the box is set"
        if name == "dev" and case.inl_pad:
            assert (got["buffer"][:, case.w:] == K.CANARY).all(), "the padding of the inlier image was written"


def test_no_inlier_image_wanted(vp):
    case = K.BY_ID["mask_cuts_runs"]
    want = K.stated(case.id)
    for got in (K.call_dev(vp, case, want_inliers=False), K.call_f32(vp.default_context().handle, case, want_inliers=False)):
        K.same_exact(got, want, case.id)
        K.same_refit(got, want, case.id)


def test_second_call_on_the_context_carries_nothing_over(vp):
    order = ["width_257_run_ends", "two_points", "usable_65", "through_origin", "outliers_90_cut_at_44", "three_points", "width_257_run_ends"]
    for cid in order:
        got = K.call_dev(vp, K.BY_ID[cid])
        K.same_exact(got, K.stated(cid), cid)
        K.same_refit(got, K.stated(cid), cid)
