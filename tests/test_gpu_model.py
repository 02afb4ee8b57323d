"""GPU suite of robust motion estimation from point pairs (vision.utils.feature.estimate_motion, cv2_facade.findHomography,
estimateAffine2D, estimateAffinePartial2D; libvp vp_model.hip): vp_estimate_model_f32 and vp_estimate_model_dev are compared bit for
bit - model, inlier mask, inlier count, hypotheses taken - with vp_estimate_model_host and with the statement tests/model_restate.py,
on the sweep of the CPU suite and at the sizes where a kernel can go wrong and a host loop cannot.  At most 10,000 points a case."""
import ctypes as C
import math

import numpy as np
import pytest

import model_cases as K
import model_restate as R

pytestmark = pytest.mark.gpu


class DevicePoints:
    """two point arrays in HBM for vp_estimate_model_dev"""

    def __init__(self, vp, src, dst):
        self.vp, self.ctx, self.ptrs = vp, vp.default_context(), []
        for a in (src, dst):
            a = np.ascontiguousarray(a, np.float32)
            p = C.c_void_p()
            vp.check(vp.lib().vp_dev_alloc(self.ctx.handle, a.nbytes, C.byref(p)), self.ctx.handle)
            self.ptrs.append(p.value)
            vp.check(vp.lib().vp_memcpy_h2d(self.ctx.handle, p.value, a.ctypes.data, a.nbytes), self.ctx.handle)

    def __enter__(self):
        return self.ptrs

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.vp.lib().vp_dev_free(self.ctx.handle, p)


def all_forms(vp, src, dst, model, what="", **kw):
    """f32, dev and host against the statement; returns the statement's answer"""
    want = K.stated(src, dst, model, **kw)
    h = vp.default_context().handle
    K.same(K.call("vp_estimate_model_host", None, src, dst, model, **kw), want, what + " host")
    K.same(K.call("vp_estimate_model_f32", h, src, dst, model, **kw), want, what + " f32")
    with DevicePoints(vp, src, dst) as (ps, pd):
        K.same(K.call("vp_estimate_model_dev", h, ps, pd, model, n=len(src), **kw), want, what + " dev")
    return want


@pytest.mark.parametrize("case", K.SWEEP, ids=K.SWEEP_IDS)
def test_device_search_is_the_statements(vp, case):
    cid, src, dst, model, kw = case
    all_forms(vp, src, dst, model, cid, **kw)


def test_one_point_is_refused(vp):
    src = np.zeros((1, 2), np.float32)
    for entry in ("vp_estimate_model_f32", "vp_estimate_model_dev"):
        rc, hb, mask, count, taken = K.call(entry, vp.default_context().handle, src, src, R.SIMILARITY)
        assert rc == vp.ERR_INVALID and "fewer point pairs" in K.library().vp_last_error(None).decode()
        assert (hb.view(np.float64) == 7.25).all() and (mask == 9).all() and (count, taken) == (-5, -5)


@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("model", K.MODELS)
def test_round_the_points_a_block_stages_at_once(vp, model, delta):
    n = K.library().vp_model_stage_points() + delta          # the plan's constant through its getter, not a copy
    src, dst, good, _ = K.pairs(n, model, 0.3)
    H, mask, count, taken, _ = all_forms(vp, src, dst, model, f"n={n}")
    assert count == good.sum() and mask[good].all()


@pytest.mark.parametrize("model", K.MODELS)
def test_ten_thousand_points_half_of_them_outliers(vp, model):
    src, dst, good, _ = K.pairs(10000, model, 0.5)
    H, mask, count, taken, _ = all_forms(vp, src, dst, model)
    assert mask[good].all() and np.abs(R.apply(H, src[good]) - dst[good]).max() < 0.01


@pytest.mark.parametrize("max_iters", [1, R.ROUND - 1, R.ROUND, R.ROUND + 1, 300, 3 * R.ROUND])
def test_round_boundaries_of_max_iters(vp, max_iters):
    """a set on which the stop table never lets go, so every hypothesis up to max_iters counts: the last round is cut, not filled"""
    for model in K.MODELS:
        src, dst, _, _ = K.pairs(65, model, (0.86, 0.75, 0.65)[model], 1)
        want = all_forms(vp, src, dst, model, max_iters=max_iters, confidence=0.999999)
        assert want[3] == max_iters


def test_a_search_that_stops_in_round_one_ignores_the_rounds_enqueued_behind_it(vp):
    h = vp.default_context().handle
    for model in K.MODELS:
        src, dst, _, _ = K.pairs(257, model, 0.0)
        long = K.call("vp_estimate_model_f32", h, src, dst, model, max_iters=2000)
        short = K.call("vp_estimate_model_f32", h, src, dst, model, max_iters=R.ROUND)
        K.same(long, K.stated(src, dst, model, max_iters=2000))
        assert long[4] == R.ROUND == short[4] and (long[1] == short[1]).all() and long[2].tobytes() == short[2].tobytes() and long[3] == short[3] == 257


def two_motions():
    """twenty integer points moved by (5, -3) and twenty others by (-7, 11): every clean sample of either group gives that group's
    exact model with exactly twenty inliers, so which group wins is the tie rule's decision alone"""
    r = np.random.default_rng(11)
    src = r.permutation(64 * 64)[:40].astype(np.int64)
    src = np.stack([src % 64 * 8, src // 64 * 8], 1).astype(np.float32)
    dst = src.copy()
    dst[:20] += np.float32([5, -3])
    dst[20:] += np.float32([-7, 11])
    return src, dst


def test_equal_counts_go_to_the_lowest_hypothesis(vp):
    src, dst = two_motions()
    winners = set()
    for seed in range(8):
        want = all_forms(vp, src, dst, R.SIMILARITY, f"seed {seed}", seed=seed, threshold=0.5)
        H, mask, count, taken, best_j = want
        assert count == 20 and (mask[:20].all() or mask[20:].all())
        first = {}
        for j in range(taken):                        # the first hypothesis of each group that reaches twenty
            s, hyp = R.hypothesis(src, dst, R.SIMILARITY, seed, j)
            group = (s[0] >= 20) if hyp is not None and (s[0] >= 20) == (s[1] >= 20) else None
            if group is not None and group not in first and R.inliers(hyp, R.SIMILARITY, src, dst, 0.25).sum() == 20:
                first[group] = j
        assert len(first) == 2 and best_j == min(first.values()) and bool(mask[20:].all()) == (first[True] < first[False])
        winners.add(bool(mask[20:].all()))
    assert winners == {False, True}, "the seeds were meant to let each group come first at least once"


def test_points_that_are_not_finite_are_never_inliers(vp):
    for model in K.MODELS:
        src, dst, good, _ = (a.copy() for a in K.pairs(300, model, 0.2, 5))
        src[3, 0], src[40, 1], dst[77, 0], dst[150, 1] = np.nan, np.inf, -np.inf, np.nan
        src[200], dst[201] = np.inf, np.nan
        broken = [3, 40, 77, 150, 200, 201]
        H, mask, count, taken, _ = all_forms(vp, src, dst, model)
        ok = good.copy()
        ok[broken] = False
        assert H is not None and not mask[broken].any() and mask[ok].all() and count == mask.sum()


def test_the_same_call_twice_and_two_seeds(vp):
    h = vp.default_context().handle
    src, dst, _, _ = K.pairs(257, R.HOMOGRAPHY, 0.6)
    a = K.call("vp_estimate_model_f32", h, src, dst, R.HOMOGRAPHY, seed=1)
    b = K.call("vp_estimate_model_f32", h, src, dst, R.HOMOGRAPHY, seed=1)
    assert a[0] == b[0] == 0 and (a[1] == b[1]).all() and a[2].tobytes() == b[2].tobytes() and a[3:] == b[3:]
    K.same(a, K.stated(src, dst, R.HOMOGRAPHY, seed=1))
    K.same(K.call("vp_estimate_model_f32", h, src, dst, R.HOMOGRAPHY, seed=2), K.stated(src, dst, R.HOMOGRAPHY, seed=2))
    assert [R.sample(257, 4, 1, j)[0] for j in range(8)] != [R.sample(257, 4, 2, j)[0] for j in range(8)]


def test_without_a_mask_pointer_the_rest_of_the_answer_is_the_same(vp):
    h = vp.default_context().handle
    for model in K.MODELS:
        src, dst, _, _ = K.pairs(257, model, 0.3)
        want = K.stated(src, dst, model)
        K.same(K.call("vp_estimate_model_f32", h, src, dst, model, want_mask=False), want)
        with DevicePoints(vp, src, dst) as (ps, pd):
            K.same(K.call("vp_estimate_model_dev", h, ps, pd, model, n=257, want_mask=False), want)


# ---- the chain: corners -> flow -> motion --------------------------------------------------------------------------------------------
CHAIN_DEGREES, CHAIN_SHIFT = 2.0, (3, -2)
# measured on an MI355X, where the statement's own answer on the tracked points is the library's bit for bit (200 corners, 200
# tracked, 199 inliers): the rotation is off by 0.04271 degrees and the image of the frame's centre by 0.04317 px - what rotate's
# bilinear resampling and the tracker leave; the bounds are twice that
CHAIN_ANGLE_MEASURED, CHAIN_SHIFT_MEASURED = 0.04271, 0.04317


def test_corners_flow_and_motion_recover_a_known_similarity(vp):
    import flow_restate
    from vision.utils import feature, transform
    a = flow_restate.texture(120, 160, 7)
    b = transform.translate(transform.rotate(a, CHAIN_DEGREES), *CHAIN_SHIFT)
    corners = feature.good_features_to_track(a, 200, 0.01, 6)
    pts = np.asarray(corners, np.float32).reshape(-1, 2)
    found, status, _ = feature.track_points(a, np.asarray(b), pts)
    assert status.sum() >= 20
    M, inl = feature.estimate_motion(pts, found, "similarity", status=status)
    kept_src, kept_dst = pts[status], found.reshape(-1, 2)[status]
    H, mask, count, taken, _ = K.stated(kept_src, kept_dst, R.SIMILARITY)
    assert M.shape == (2, 3) and M.dtype == np.float64 and (M.reshape(-1).view(np.uint64) == R.bits(H)[:6]).all() and inl.tobytes() == (mask != 0).tobytes()
    # cv2's rotation about the centre, counter-clockwise on the screen, then the shift
    t = math.radians(CHAIN_DEGREES)
    ca, sa, cx, cy = math.cos(t), math.sin(t), 80.0, 60.0
    truth = np.array([[ca, sa, (1 - ca) * cx - sa * cy + CHAIN_SHIFT[0]], [-sa, ca, sa * cx + (1 - ca) * cy + CHAIN_SHIFT[1]]])
    angle_off = abs(math.degrees(math.atan2(M[1, 0], M[0, 0]) - math.atan2(truth[1, 0], truth[0, 0])))
    centre_off = float(np.abs(M @ [cx, cy, 1.0] - truth @ [cx, cy, 1.0]).max())
    print(f"chain: {int(status.sum())} tracked of {len(pts)}, {count} inliers, rotation off by {angle_off:.4g} degrees, the centre's image off by {centre_off:.4g} px")
    assert angle_off <= 2 * CHAIN_ANGLE_MEASURED and centre_off <= 2 * CHAIN_SHIFT_MEASURED


# ---- the facade ------------------------------------------------------------------------------------------------------------------------
def test_facade_shapes_types_and_no_model(vp):
    from vision import cv2_facade as f
    src, dst, good, _ = K.pairs(257, R.HOMOGRAPHY, 0.3)
    H, mask = f.findHomography(src.reshape(-1, 1, 2), dst.reshape(-1, 1, 2), f.RANSAC, 3.0, None)
    assert H.shape == (3, 3) and H.dtype == np.float64 and mask.shape == (257, 1) and mask.dtype == np.uint8 and H[2, 2] == 1.0
    want = K.stated(src, dst, R.HOMOGRAPHY, confidence=0.995)
    assert (H.reshape(-1).view(np.uint64) == R.bits(want[0])).all() and mask.reshape(-1).tobytes() == want[1].tobytes()
    given = np.zeros((257, 1), np.uint8)
    assert f.findHomography(src, dst, f.RANSAC, 3.0, given)[1] is given and given.reshape(-1).tobytes() == want[1].tobytes()
    for fn, model in ((f.estimateAffine2D, R.AFFINE), (f.estimateAffinePartial2D, R.SIMILARITY)):
        s, d, _, _ = K.pairs(257, model, 0.3)
        M, inl = fn(s, d)
        want = K.stated(s, d, model)
        assert M.shape == (2, 3) and M.dtype == np.float64 and inl.shape == (257, 1) and inl.dtype == np.uint8
        assert (M.reshape(-1).view(np.uint64) == R.bits(want[0])[:6]).all() and inl.reshape(-1).tobytes() == want[1].tobytes()
        assert fn(s, d, None, f.RANSAC, 3.0, 2000, 0.99, 10)[0].tobytes() == M.tobytes()
        with pytest.raises(f.error):
            fn(s, d, method=f.LMEDS)
        with pytest.raises(f.error):
            fn(s, d, method=f.RHO)
    same_point = np.full((40, 2), 7.5, np.float32)
    assert f.findHomography(same_point, same_point, f.RANSAC) == (None, None)
    assert f.estimateAffine2D(same_point, same_point) == (None, None) and f.estimateAffinePartial2D(same_point, same_point) == (None, None)
    for method in (f.LMEDS, f.RHO):
        with pytest.raises(f.error):
            f.findHomography(src, dst, method)
