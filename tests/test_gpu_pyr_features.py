"""GPU suite of the features over a scale pyramid (vision.utils.feature.pyramid_features, vision.utils.sift.PyramidSIFT; libvp
vp_pyr_features_*).  Every case is compared byte for byte with the statement tests/pyr_features_restate.py -
points, levels, scores, bins, descriptors and order - at the sizes where a kernel can go wrong: sides round the level cut-off and the
tile width on level 0 and below, budgets round every level's quota, equal scores at the cutoff, and both forms of the entry.  The
recognition test is the one the feature exists for: a source found at half, at one and at twice its size."""
import ctypes as C

import numpy as np
import pytest

import features_cases as K
import features_restate as R
import pyr_features_cases as PC
import pyr_features_restate as P

pytestmark = pytest.mark.gpu


class DeviceBytes:
    """host arrays copied into HBM for the _dev entry"""

    def __init__(self, vp, *arrays):
        self.vp, self.ctx, self.ptrs = vp, vp.default_context(), []
        for a in arrays:
            a = np.ascontiguousarray(a)
            p = C.c_void_p()
            vp.check(vp.lib().vp_dev_alloc(self.ctx.handle, max(a.nbytes, 8), C.byref(p)), self.ctx.handle)
            self.ptrs.append(p.value)
            vp.check(vp.lib().vp_memcpy_h2d(self.ctx.handle, p.value, a.ctypes.data, a.nbytes), self.ctx.handle)

    def __enter__(self):
        return self.ptrs

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.vp.lib().vp_dev_free(self.ctx.handle, p)


def budget_with_quota(sizes, level, want):
    """the smallest budget at which the level's quota is `want`"""
    return next(n for n in range(1 << 16) if P.quotas(sizes, n)[level] == want)


def forms(vp, img, threshold, max_points, levels=8, pad=5):
    """[(n, xy0, lxy, score, bin, desc)] of vp_pyr_features_u8 (packed rows) and vp_pyr_features_dev (rows padded by `pad` bytes)"""
    img = np.ascontiguousarray(img)
    h, w = img.shape
    wide = np.full((h, w + pad), 201, np.uint8)
    wide[:, :w] = img
    cap = max(max_points, 1)
    out = []
    ctx = vp.default_context()
    with DeviceBytes(vp, wide) as (d_src,):
        for entry, src, stride in ((vp.lib().vp_pyr_features_u8, img.ctypes.data, w), (vp.lib().vp_pyr_features_dev, d_src, w + pad)):
            xy0, lxy, val = np.full((cap, 2), -9, np.float32), np.full((cap, 3), -9, np.int32), np.full(cap, -9, np.int32)
            bins, desc, n = np.full(cap, 9, np.uint8), np.full((cap, 32), 9, np.uint8), C.c_int(-9)
            vp.check(entry(ctx.handle, src, stride, w, h, levels, threshold, max_points, xy0.ctypes.data, lxy.ctypes.data, val.ctypes.data, bins.ctypes.data,
                           desc.ctypes.data, None, C.addressof(n)), ctx.handle)
            out.append((n.value, xy0, lxy, val, bins, desc))
    return out


def check(vp, img, threshold, max_points, levels=8):
    want = P.pyramid_features(img, threshold, max_points, levels)
    pts0, desc, lev, score, bins, lxy = want
    for n, g_xy0, g_lxy, g_val, g_bins, g_desc in forms(vp, img, threshold, max_points, levels):
        assert n == len(pts0) <= max_points, (img.shape, threshold, max_points, levels, n, len(pts0))
        assert np.array_equal(g_lxy[:n], lxy), "levels, positions or order"
        assert g_xy0[:n].tobytes() == pts0.tobytes(), "level-0 coordinates"
        assert np.array_equal(g_val[:n], score) and np.array_equal(g_bins[:n], bins) and np.array_equal(g_desc[:n], desc)
    return want


@pytest.mark.parametrize("threshold", [5, 20])
@pytest.mark.parametrize("shape", [(30, 40), (31, 31), (36, 37), (37, 37), (45, 64), (47, 65), (97, 131)])
def test_image_sides_round_the_level_cutoff_and_the_tile(vp, shape, threshold):
    img = PC.soft_noise(shape[0], shape[1], 5)
    want = check(vp, img, threshold, 2000)
    sizes = P.level_sizes(shape[1], shape[0], 8)
    if shape == (30, 40):
        assert sizes == [] and len(want[0]) == 0
    if shape == (97, 131) and threshold == 5:
        assert len(sizes) == 7 and len(set(want[2].tolist())) >= 4, "corners on several levels"


def test_one_level_is_fast_corners_then_describe_points(vp):
    from vision.devmat import DeviceMat
    from vision.utils import feature
    img = np.ascontiguousarray(PC.soft_noise(97, 131, 5))
    h, w = img.shape
    for max_points in (40, 100000):
        # fast_corners caps over the whole image; the statement caps among the describable corners: compare uncapped, cap by the statement's rule
        pts, scores = feature.fast_corners(img, 5, True)
        ok = (pts[:, 0] >= 15) & (pts[:, 0] <= w - 16) & (pts[:, 1] >= 15) & (pts[:, 1] <= h - 16)
        xy, sc = R.top_points(pts[ok].astype(np.int32), scores[ok], max_points)
        kept, des, index = feature.describe_points(img, xy.astype(np.float32))
        assert len(index) == len(xy)
        for mat in (img, DeviceMat.from_host(vp.default_context(), img)):
            pts0, d, lev, s, b = feature.pyramid_features(mat, 5, max_points, levels=1)
            assert np.array_equal(pts0, kept) and np.array_equal(d, des) and np.array_equal(s, sc) and (lev == 0).all() and len(b) == len(d)
            assert pts0.dtype == np.float32 and d.dtype == np.uint8 and lev.dtype == np.int32 and s.dtype == np.int32 and b.dtype == np.uint8


def test_budgets_round_every_quota(vp):
    img = PC.soft_noise(97, 131, 5)
    sizes = P.level_sizes(131, 97, 8)
    found = [len(P.level_candidates(L, 5)[0]) for L in P.build_levels(img, 8)]
    assert all(found), found
    budgets = {0, 1, 3}                                   # 3: q_l == 0 on the small levels
    assert 0 in P.quotas(sizes, 3)[1:]
    total_cap = 1 << 16
    assert all(q >= f for q, f in zip(P.quotas(sizes, total_cap), found)), "a budget above everything found"
    budgets.add(total_cap)
    for l, f in enumerate(found):
        # the budgets at which level l's quota is one below, at, and one above what it found
        for want_q in (f - 1, f, f + 1):
            budgets.add(budget_with_quota(sizes, l, want_q))
    for n in sorted(budgets):
        want = check(vp, img, 5, n)
        if n == total_cap:
            assert len(want[0]) == sum(found)


def test_equal_scores_at_the_cutoff_keep_the_earliest_in_the_raster(vp):
    img = PC.dot_tiling(168, 168)
    sizes = P.level_sizes(168, 168, 8)
    xy, sc = P.level_candidates(np.asarray(img), 20)
    assert len(xy) == 289 and (sc == 99).all(), "17 x 17 identical corners on level 0"
    for want_q0 in (30, 100, 270, 288, 289):              # inside the first wave's run, inside a later one, past the 256th, the last
        n = budget_with_quota(sizes, 0, want_q0)
        pts0, desc, lev, score, bins, lxy = check(vp, img, 20, n)
        level0 = lxy[lev == 0]
        assert len(level0) == want_q0 and np.array_equal(level0[:, 1:], xy[:want_q0]), "the earliest in raster order"


@pytest.mark.parametrize("train_count", [1, 127, 129])
def test_device_descriptors_match_as_the_host_arrays_do(vp, train_count):
    from vision.devmat import DeviceMat
    from vision.utils import feature
    ctx = vp.default_context()
    a, b = np.ascontiguousarray(PC.soft_noise(97, 131, 5)), np.ascontiguousarray(PC.soft_noise(97, 131, 6))
    # a small level may find less than its quota: the first budget that gives exactly train_count points
    budget = next(n for n in range(train_count, train_count + 16) if len(feature.pyramid_features(b, 5, n)[0]) == train_count)
    qa = feature.pyramid_features(a, 5, 300, device_descriptors=True)
    tb = feature.pyramid_features(DeviceMat.from_host(ctx, b), 5, budget, device_descriptors=True)
    ha, hb = feature.pyramid_features(a, 5, 300), feature.pyramid_features(b, 5, budget)
    assert isinstance(qa[1], DeviceMat) and isinstance(tb[1], DeviceMat) and qa[1].shape == ha[1].shape and tb[1].shape == (train_count, 32)
    assert np.array_equal(qa[1].host_copy(), ha[1]) and np.array_equal(tb[1].host_copy(), hb[1])
    assert np.array_equal(ha[1], P.pyramid_features(a, 5, 300)[1])
    for k, cross in ((2, False), (1, False), (1, True)):
        idx, dist = feature.match_descriptors(qa[1], tb[1], k, cross)
        hidx, hdist = feature.match_descriptors(ha[1], hb[1], k, cross)
        ridx, rdist = R.hamming_knn(ha[1], hb[1], k, cross)
        assert idx.dtype == np.int32 and np.array_equal(idx, hidx) and np.array_equal(dist, hdist)
        assert np.array_equal(idx, ridx) and np.array_equal(dist[ridx >= 0], rdist[ridx >= 0])


def test_a_source_is_found_at_half_at_one_and_at_twice_its_size(vp):
    from vision import cv2_facade as f
    from vision.devmat import DeviceMat
    from vision.utils import feature
    from vision.utils.sift import SIFT, PyramidSIFT
    ctx = vp.default_context()
    tex = np.ascontiguousarray(PC.texture())
    src = PC.stated_features("source")
    sizes = P.level_sizes(PC.TEX_W, PC.TEX_H, PC.LEVELS)
    single = SIFT()
    single.add_source("texture", tex)
    for make in (lambda a: a, lambda a: DeviceMat.from_host(ctx, a)):
        s = PyramidSIFT()
        kp, des = s.add_source("texture", make(tex))
        assert [k.pt for k in kp] == [tuple(map(float, p)) for p in src[0]] and np.array_equal(des, src[1])
        assert [k.octave for k in kp] == src[2].tolist() and [k.response for k in kp] == src[3].astype(float).tolist()
        assert [k.angle for k in kp] == [11.25 * int(b) for b in src[4]]
        assert [k.size for k in kp] == [float(P.keypoint_size(PC.TEX_W, sizes[l][0])) for l in src[2]]
        for which in PC.SCALES:
            frame, true = PC.scene(which)
            frame = np.ascontiguousarray(frame)
            want, feat = PC.stated_recognition(which), PC.stated_features(which)
            assert want["H"] is not None and want["inliers"] >= K.MIN_MATCH, "the statement itself must find the source at this scale"
            matched, fkp, fdes = s.match(make(frame))
            assert [k.pt for k in fkp] == [tuple(map(float, p)) for p in feat[0]] and np.array_equal(fdes, feat[1]) and [k.octave for k in fkp] == feat[2].tolist()
            assert len(matched) == 1, which
            name, good, dst, mask, drawn = matched[0]
            assert name == "texture" and drawn is None
            assert [(m.queryIdx, m.trainIdx, m.distance) for m in good] == [(int(a), int(b), float(want["dist"][a, 0])) for a, b in zip(want["q"], want["t"])]
            assert mask == [int(v != 0) for v in want["mask"]] and sum(mask) >= K.MIN_MATCH
            assert dst.dtype == np.int32 and dst.shape == (4, 1, 2) and np.array_equal(dst, want["dst"])
            H, inliers = feature.estimate_motion(src[0][want["q"]], feat[0][want["t"]], model="homography", threshold=K.RANSAC_THRESHOLD)
            assert H.tobytes() == want["H"].tobytes() and np.array_equal(inliers, want["mask"] != 0), "the homography, bit for bit"
            proj = f.perspectiveTransform(np.float64(PC.SOURCE_CORNERS).reshape(-1, 1, 2), H).reshape(4, 2)
            err = float(np.sqrt(((proj - true) ** 2).sum(axis=1)).max())
            print("%s: %d good, %d inliers, largest corner error %.4f px (the statement: %.4f, bound %.4f)" % (which, len(good), sum(mask), err,
                                                                                                             PC.CORNER_ERROR_MEASURED[which], PC.CORNER_ERROR_BOUND))
            assert err <= PC.CORNER_ERROR_BOUND
            if which != "turned":                         # for contrast only: the single-scale class on the same frame
                print("%s: single-scale SIFT reports %d source(s)" % (which, len(single.match(frame)[0])))
