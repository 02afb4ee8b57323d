"""CPU suite for stereo block matching: vp_stereo_bm_host and vp_depth_from_disparity_host (scalar C++ inside libvp, no device) equal
tests/stereo_restate.py byte for byte over every case the GPU test walks, and the statement itself has the properties a matcher must
have - a shifted scene is found, flat and periodic scenes are refused, nothing outside the candidate rectangle is answered."""
import numpy as np
import pytest

import stereo_cases as SC
import stereo_restate as R

CASES = SC.cases(SC.lib_plan)
FOCAL, BASELINE = 534.48, 0.12


def _host_depth(disp, focal, baseline):
    from vision import _vp
    h, w = disp.shape
    out = np.empty((h, w), np.float32)
    _vp.check(_vp.lib().vp_depth_from_disparity_host(disp.ctypes.data, 2 * w, w, h, focal, baseline, out.ctypes.data, 4 * w))
    return out


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_host_routine_equals_the_statement(case):
    left, right = case["pair"]()
    want = SC.expected(case)
    got = SC.host_disparity(left, right, **case["params"])
    assert got.dtype == np.int16 and np.array_equal(got, want), f"{int((got != want).sum())} pixels differ"
    depth = _host_depth(np.ascontiguousarray(want), FOCAL, BASELINE)
    assert depth.tobytes() == R.depth_from_disparity(want, FOCAL, BASELINE).tobytes()


def _candidates(out, params):
    x, y, w, h = R.valid_rect(out.shape[1], out.shape[0], params["num_disparities"], params["block_size"], params["min_disparity"])
    return out[y:y + h, x:x + w]


@pytest.mark.parametrize("d0,n,bs,m", [(9, 32, 9, 0), (3, 16, 5, 0), (40, 64, 15, 0), (-5, 16, 7, -12), (130, 16, 11, 120)])
def test_shifted_pair_is_found(d0, n, bs, m):
    left, right = SC.shifted_pair(48, 260, d0, seed=11)
    p = dict(num_disparities=n, block_size=bs, min_disparity=m)
    out = R.disparity(left, right, **p)
    cand = _candidates(out, {**R.DEFAULTS, **p})
    found = cand[cand != R.invalid_disparity(m)]
    assert cand.size and found.size * 2 >= cand.size          # an all-invalid result can never pass for a match
    assert np.all(np.abs(found.astype(np.int32) - 16 * d0) <= 8)
    # the scene matches itself exactly at d0 wherever the window is clear of the prefilter's constant border columns: C* = 0 there, so
    # the offset |pm - pp| 256 / (pm + pp + |pm - pp|) is at most 128 and the result is within 8 of 16 d0
    C, _, _ = R.cost_volume(left, right, n, bs, m, 31)
    assert np.all(C[d0 - m][:, 1:-1] == 0)


def test_every_generated_shift_keeps_half_of_its_candidates():
    for case in CASES:
        if case["id"].startswith(("strip_", "block_", "nd_", "min_", "hd720")) or case["id"] in ("rows_h10", "uniq_0"):
            cand = _candidates(SC.expected(case), case["params"])
            assert cand.size and (cand != R.invalid_disparity(case["params"]["min_disparity"])).sum() * 2 >= cand.size, case["id"]


def test_flat_pair_is_all_invalid_unless_texture_is_not_asked_for():
    img = SC.flat(40, 120)
    assert np.all(R.disparity(img, img, num_disparities=32, block_size=9, texture_threshold=10) == -16)
    free = R.disparity(img, img, num_disparities=32, block_size=9, texture_threshold=0, uniqueness_ratio=0)
    cand = _candidates(free, dict(num_disparities=32, block_size=9, min_disparity=0))
    assert np.all(cand == 31 * 16)                            # every cost is 0: the tie goes to the largest disparity, offset 0


def test_stripes_are_refused_by_uniqueness_and_tie_to_the_larger_disparity():
    img = SC.stripes(40, 120, 8)
    p = dict(num_disparities=32, block_size=9)                # four periods fit the range
    # (the first and last candidate columns have a window on one of the prefilter's constant border columns, which are not periodic)
    refused = _candidates(R.disparity(img, img, **p, uniqueness_ratio=15), dict(**p, min_disparity=0))
    assert refused.size and np.all(refused[:, 1:-1] == -16)
    cand = _candidates(R.disparity(img, img, **p, uniqueness_ratio=0), dict(**p, min_disparity=0))
    # costs vanish at 0, 8, 16 and 24: D* is 24, the largest of them, and the subpixel offset stays within half a disparity of it
    assert cand.size and np.all(np.abs(cand[:, 1:-1].astype(np.int32) - 24 * 16) <= 8)
    C, _, _ = R.cost_volume(img, img, 32, 9, 0, 31)
    assert all(np.all(C[d][:, 1:-1] == 0) for d in (0, 8, 16, 24)) and np.all(C[23] > 0) and np.all(C[25] > 0)


def test_outside_the_rectangle_everything_is_invalid():
    left, right = SC.shifted_pair(40, 200, 6, seed=12)
    for m, n, bs in ((0, 16, 9), (-3, 32, 5), (4, 16, 21), (0, 16, 5)):
        out = R.disparity(left, right, num_disparities=n, block_size=bs, min_disparity=m, texture_threshold=0, uniqueness_ratio=0)
        x, y, w, h = R.valid_rect(200, 40, n, bs, m)
        mask = np.ones(out.shape, bool)
        mask[y:y + h, x:x + w] = False
        assert w * h > 0 and np.all(out[mask] == (m - 1) * 16) and np.all(out[~mask] != (m - 1) * 16)
    assert R.valid_rect(19, 5, 16, 5, 0) == (0, 0, 0, 0) and R.valid_rect(20, 5, 16, 5, 0) == (17, 2, 1, 1)
    assert R.invalid_disparity(0) == -16 and R.invalid_disparity(-128) == -2064


def test_depth_is_the_stated_double_quotient():
    left, right = SC.two_plane_pair(40, 160, 7)
    disp = R.disparity(left, right, num_disparities=16, block_size=9)
    z = R.depth_from_disparity(disp, FOCAL, BASELINE)
    assert z.dtype == np.float32 and np.all(z[disp <= 0] == 0) and np.any(disp == -16)
    fb = FOCAL * BASELINE
    for v in np.unique(disp[disp > 0]):
        assert np.all(z[disp == v] == np.float32(fb * 16.0 / float(v)))
    # both planes are there, at their depths
    assert np.float32(fb / 5.0) in z and np.float32(fb / 11.0) in z
    assert np.count_nonzero(disp == 80) > 200 and np.count_nonzero(disp == 176) > 200
