"""CPU suite: the HoughCircles statement of the tests (hough_circles_restate.py) checked step by step against hand-worked cases and
geometry, and the facade's signature and argument checks (which raise before libvp is called)."""
import inspect

import numpy as np
import pytest

import hough_circles_restate as HC


def discs(seed, h, w, circles, noise=6):
    """Anti-aliased bright discs on a dark noisy ground, 5x5 binomial blur (a hard-edged disc's staircase scatters the gradients)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    img = 30 + rng.random((h, w)) * noise
    for cx, cy, r in circles:
        cov = np.clip(r - np.hypot(xx - cx, yy - cy) + 0.5, 0, 1)
        img = img * (1 - cov) + 200 * cov
    k = np.array([1, 4, 6, 4, 1], np.float64) / 16
    p = np.pad(img, 2, mode="edge")
    img = sum(k[i] * p[:, i:i + w] for i in range(5))
    img = sum(k[i] * img[i:i + h, :] for i in range(5))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _cells(acc, acols):
    idx = np.flatnonzero(acc)
    return sorted((int(i) // (acols + 2), int(i) % (acols + 2), int(acc[i])) for i in idx)


def test_one_ray_by_hand():
    # a pixel at (5, 4) with gradient (3, 4): sx = cvRound(3 * 1024 / 5) = 614, sy = 819; x0 = 5120, y0 = 4096; acc 10 x 8
    sx, sy, x0, y0 = HC.ray_params(np.array([5]), np.array([4]), np.float32([3]), np.float32([4]), np.float32([5]), np.float32(1))
    assert (sx[0], sy[0], x0[0], y0[0]) == (614, 819, 5120, 4096)
    acc = np.zeros(12 * 10, np.int64)
    HC.vote(acc, 10, 8, sx, sy, x0, y0, 0, 20)
    exp = {}
    for sign in (1, -1):
        for r in range(0, 21):
            x2, y2 = (5120 + r * sign * 614) >> 10, (4096 + r * sign * 819) >> 10
            if not (0 <= x2 < 10 and 0 <= y2 < 8):
                break
            exp[(y2 + 1, x2 + 1)] = exp.get((y2 + 1, x2 + 1), 0) + 1
    # worked out: + direction r = 0..5 (unbordered cells (5,4) (5,4) (6,5) (6,6) (7,7) (7,7)), r = 6 leaves at y2 = 8; - direction
    # r = 0..5 ((5,4) (4,3) (3,2) (3,1) (2,0) (2,0)), r = 6 leaves at y2 = -1.  Keys: bordered (row, column).
    assert exp == {(5, 6): 3, (6, 7): 1, (7, 7): 1, (8, 8): 2, (4, 5): 1, (3, 4): 1, (2, 4): 1, (1, 3): 2}
    assert _cells(acc, 10) == sorted((y, x, v) for (y, x), v in exp.items())
    assert acc.sum() == 12


def test_min_radius_start_outside_votes_nothing():
    sx, sy, x0, y0 = np.array([1024]), np.array([0]), np.array([2048]), np.array([1024])
    acc = np.zeros(12 * 10, np.int64)
    HC.vote(acc, 10, 8, sx, sy, x0, y0, 9, 30)           # + : x2 = 11 at r = 9, outside at once; - : x2 = -7, outside
    assert not acc.any()
    HC.vote(acc, 10, 8, sx, sy, x0, y0, 2, 30)           # + : r = 2..7 (x2 = 4..9); - : r = 2 only (x2 = 0)
    assert acc.sum() == 7


def test_stop_at_first_outside_equals_skip_outside():
    """The cells of a ray are monotone in r and the ray starts inside at r = 0, so OpenCV's early stop votes the same set of cells as
    voting every inside cell - what lets the GPU count a tile's r interval without walking from minRadius."""
    rng = np.random.default_rng(3)
    for dp in (1.0, 1.5, 2.0):
        h, w = 37, 53
        idp = np.float32(1) / np.float32(dp)
        arows, acols = HC.accum_size((h, w), idp)
        n = 400
        xs, ys = rng.integers(0, w, n), rng.integers(0, h, n)
        vx, vy = rng.integers(-400, 401, n).astype(np.float32), rng.integers(-400, 401, n).astype(np.float32)
        keep = (vx != 0) | (vy != 0)
        xs, ys, vx, vy = xs[keep], ys[keep], vx[keep], vy[keep]
        mag = np.sqrt(vx * vx + vy * vy)
        sx, sy, x0, y0 = HC.ray_params(xs, ys, vx, vy, mag, idp)
        for lo, hi in ((0, 60), (5, 12), (30, 31)):
            a = np.zeros((arows + 2) * (acols + 2), np.int64)
            HC.vote(a, acols, arows, sx, sy, x0, y0, lo, hi)
            b = np.zeros_like(a)
            r = np.arange(lo, hi + 1)
            for sign in (1, -1):
                x2 = (x0[:, None] + r * sign * sx[:, None]) >> 10
                y2 = (y0[:, None] + r * sign * sy[:, None]) >> 10
                m = (x2 >= 0) & (x2 < acols) & (y2 >= 0) & (y2 < arows)
                b += np.bincount(((y2[m] + 1) * (acols + 2) + x2[m] + 1), minlength=b.size)
            assert np.array_equal(a, b), (dp, lo, hi)


def test_centre_rule_and_tie_order():
    acc = np.zeros((6, 7), np.int64)
    acc[2, 2] = 5; acc[2, 3] = 5                          # equal right neighbour: the left one is a centre, the right one is not
    acc[4, 5] = 5; acc[3, 5] = 5                          # equal upper neighbour: the upper one is a centre, the lower one is not
    acc[4, 2] = 7
    acc[1, 5] = 2                                         # not above the threshold 2
    ofs, votes = HC.centres(acc, 2)
    assert ofs.tolist() == [4 * 7 + 2, 2 * 7 + 2, 3 * 7 + 5] and votes.tolist() == [7, 5, 5]


def test_bin_walk_by_hand():
    dp, mr = np.float32(1), 0
    # one non-empty bin at 25: the group is 25..16, j ends at 15, rCur = (25 + 15) / 2 / 10 = 2.0
    b = np.zeros(40, np.int64); b[25] = 3
    assert HC.walk_bins(b, mr, dp) == (3, np.float32(2.0))
    # rBest = 0 takes the first group (FLT_EPSILON clause); a later group wins when curCount * rBest >= maxCount * rCur
    b = np.zeros(40, np.int64); b[35] = 2; b[12] = 3
    m, r = HC.walk_bins(b, mr, dp)
    r1 = np.float32(np.float32(35 + 25) / np.float32(2)) / np.float32(10)
    r2 = np.float32(np.float32(12 + 2) / np.float32(2)) / np.float32(10)
    assert (m, r) == ((3, r2) if np.float32(3) * r1 >= np.float32(2) * r2 else (2, r1))
    # a group that reaches bin 0: j ends at -1; bin 0 alone is never opened (the loop stops at j > 0)
    b = np.zeros(20, np.int64); b[4] = 1; b[0] = 5
    assert HC.walk_bins(b, mr, dp) == (6, np.float32(np.float32(4 - 1) / np.float32(2) / np.float32(10)))
    b = np.zeros(20, np.int64); b[0] = 9
    assert HC.walk_bins(b, mr, dp) == (0, np.float32(0))
    # the bin right below a group (upbin - 10) is skipped by the outer loop's own decrement
    b = np.zeros(40, np.int64); b[30] = 1; b[20] = 4
    m, _ = HC.walk_bins(b, mr, dp)
    assert m == 1
    # minRadius and dp enter rCur
    b = np.zeros(40, np.int64); b[30] = 2
    assert HC.walk_bins(b, 7, np.float32(1.5))[1] == np.float32(np.float32(np.float32(50) / np.float32(2)) / np.float32(10)) * np.float32(1.5) + np.float32(7)


def test_overlap_pass():
    c = [(np.float32(10), np.float32(10), np.float32(5)), (np.float32(14), np.float32(10), np.float32(5)),
         (np.float32(20), np.float32(10), np.float32(5)), (np.float32(10), np.float32(16), np.float32(5))]
    assert HC.remove_overlaps(c, 5) == [c[0], c[2], c[3]]
    assert HC.remove_overlaps(c, 4) == c                  # distance 4 is not below minDist 4
    assert HC.remove_overlaps(c, 100) == [c[0]]
    assert HC.remove_overlaps(c[:1], 1000) == c[:1]


def test_order_is_cmp_accum():
    e = [(np.float32(5), np.float32(5), np.float32(3), 10), (np.float32(4), np.float32(9), np.float32(3), 10),
         (np.float32(4), np.float32(2), np.float32(3), 10), (np.float32(1), np.float32(1), np.float32(8), 10), (np.float32(0), np.float32(0), np.float32(1), 12)]
    assert [x[:2] for x in HC.order(e)] == [(0, 0), (1, 1), (4, 2), (4, 9), (5, 5)]


@pytest.mark.parametrize("dp", [1, 1.5, 2])
def test_discs_come_back(dp):
    truth = ((80, 70, 30), (220, 150, 45), (270, 50, 18))
    img = discs(1, 240, 320, truth)
    got = HC.hough_circles(img, dp, 20, 100, 20, 10, 80)
    assert got is not None
    for cx, cy, r in truth:
        d = np.hypot(got[0, :, 0] - cx, got[0, :, 1] - cy)
        k = int(np.argmin(d))
        # the centre is the middle of an accumulator cell (x + 0.5) * dp; the radius the middle of a group of ten 1/10-dp bins
        assert d[k] <= 1.5 * dp + 0.5 and abs(got[0, k, 2] - r) <= 2 * dp, (cx, cy, r, got[0, k])


def test_argument_rules():
    a = HC.arguments((100, 200), 0.5, 10)
    assert a["dp"] == 1 and a["idp"] == 1 and a["max_radius"] == 200 and a["min_radius"] == 0
    assert (a["canny_low"], a["canny_high"], a["acc_thresh"]) == (50, 100, 100)
    a = HC.arguments((100, 200), 1.5, 10, 3, 2.5, -4, 0)
    assert a["dp"] == np.float32(1.5) and a["idp"] == np.float32(1) / np.float32(1.5)
    assert (a["canny_low"], a["canny_high"], a["acc_thresh"], a["min_radius"], a["max_radius"]) == (1, 3, 2, 0, 200)
    assert HC.arguments((10, 10), 1, 1, 100, 100, 20, 20)["max_radius"] == 22
    assert HC.arguments((10, 10), 1, 1, 100, 100, 20, 5)["max_radius"] == 22
    assert HC.arguments((10, 10), 1, 1, 100, 100, 3, 9)["max_radius"] == 9
    assert HC.arguments((10, 10), 1, 1, 100, 100, 30, 0)["max_radius"] == 10     # the default is not adjusted
    assert HC.n_bins(HC.arguments((10, 10), 1, 1, 100, 100, 30, 0)) < 0
    assert HC.hough_circles(np.zeros((10, 10), np.uint8), 1, 1, 100, 100, 30, 0, canny=lambda i, l, h: np.full_like(i, 255)) is None
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, -1)):
        with pytest.raises(HC.ArgumentError):
            HC.arguments((10, 10), *bad)
    with pytest.raises(NotImplementedError):
        HC.arguments((10, 10), 1, 1, 100, 100, 0, -1)


def test_facade_signature_and_checks():
    from vision import cv2_facade
    params = list(inspect.signature(cv2_facade.HoughCircles).parameters.items())
    assert [p for p, _ in params] == ["image", "method", "dp", "minDist", "circles", "param1", "param2", "minRadius", "maxRadius"]
    assert [v.default for _, v in params[4:]] == [None, 100, 100, 0, 0]
    assert (cv2_facade.HOUGH_GRADIENT, cv2_facade.HOUGH_GRADIENT_ALT) == (3, 4)
    img = np.zeros((16, 16), np.uint8)
    bad = [((img, cv2_facade.HOUGH_GRADIENT_ALT, 1.5, 10), {}), ((img, 7, 1, 10), {}),
           ((img, cv2_facade.HOUGH_GRADIENT, 1, 10), {"maxRadius": -1}), ((img, cv2_facade.HOUGH_GRADIENT, 0, 10), {}),
           ((img, cv2_facade.HOUGH_GRADIENT, 1, 0), {}), ((img, cv2_facade.HOUGH_GRADIENT, 1, 10), {"param1": 0}),
           ((img, cv2_facade.HOUGH_GRADIENT, 1, 10), {"param2": -3}), ((img.astype(np.float32), cv2_facade.HOUGH_GRADIENT, 1, 10), {}),
           ((np.zeros((16, 16, 3), np.uint8), cv2_facade.HOUGH_GRADIENT, 1, 10), {}), ((np.zeros((0, 5), np.uint8), cv2_facade.HOUGH_GRADIENT, 1, 10), {})]
    for args, kw in bad:
        with pytest.raises(cv2_facade.error):
            cv2_facade.HoughCircles(*args, **kw)


def test_find_circles_still_outside_and_hough_circles_exported():
    from vision import _vp
    from vision.utils import feature
    with pytest.raises(NotImplementedError):
        feature.find_circles(np.zeros((4, 4), np.uint8))
    assert callable(feature.hough_circles)
    assert {"vp_hough_circles_u8", "vp_hough_circles_dev"} <= set(_vp.exported_symbols())
    assert _vp.OPT_HOUGH_CIRCLES_LDS == 6 and _vp.HOUGH_GRADIENT == 3
