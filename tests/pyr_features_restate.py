"""A plain numpy statement of the features over a scale pyramid, written from the definition and not from the
library's source: the level sizes, the levels themselves (resize_restate.resize, each from the one before), the candidates of a level
(features_restate.fast among the pixels that can be described), the budget of each level, the description on the point's own level
and the coordinates reported.  All integers, or IEEE double in the stated order.  Slow and obvious on purpose."""
import numpy as np

import features_restate as R
import resize_restate as Z

MIN_SIDE, BORDER, MAX_LEVELS = 31, 15, 8


def level_sizes(w, h, levels):
    """[(w_l, h_l)]: w_l = (5 w_{l-1} + 3) // 6; the levels with both sides at least 31, at most `levels` of them"""
    assert 1 <= levels <= MAX_LEVELS
    out = []
    while len(out) < levels and min(w, h) >= MIN_SIDE:
        out.append((w, h))
        w, h = (5 * w + 3) // 6, (5 * h + 3) // 6
    return out


def quotas(sizes, max_points):
    """q_l = (N a_l) // A for l >= 1 (Python integers), q_0 the rest"""
    if not sizes:
        return []
    areas = [w * h for w, h in sizes]
    q = [0] + [(max_points * a) // sum(areas) for a in areas[1:]]
    q[0] = max_points - sum(q)
    return q


def build_levels(img, levels):
    img = np.ascontiguousarray(img)
    h, w = img.shape
    out = []
    for lw, lh in level_sizes(w, h, levels):
        out.append(img if not out else Z.resize(out[-1], (lw, lh)))
    return out


def blurred(img):
    from oracle import oracle as orc
    return orc.gaussian_blur(np.ascontiguousarray(img), (7, 7), 2.0, 2.0)


def level_candidates(level, threshold):
    """FAST-9 with suppression on the whole level, then only the corners that can be described: (xy, score) in raster order"""
    h, w = level.shape
    xy, score = R.fast(level, threshold, True)
    ok = (xy[:, 0] >= BORDER) & (xy[:, 0] <= w - 1 - BORDER) & (xy[:, 1] >= BORDER) & (xy[:, 1] <= h - 1 - BORDER)
    return xy[ok], score[ok]


def map_to_image(v, side0, side_l):
    """(float32)(((double)v + 0.5) * ((double)side0 / side_l) - 0.5), one rounding per operation"""
    ratio = np.float64(side0) / np.float64(side_l)
    return ((np.asarray(v, np.float64) + 0.5) * ratio - 0.5).astype(np.float32)


def pyramid_features(img, threshold=20, max_points=2000, levels=8):
    """(pts0 float32 (n, 2), desc uint8 (n, 32), level int32 (n,), score int32 (n,), bin uint8 (n,), lxy int32 (n, 3)) ordered by level, y, x"""
    img = np.ascontiguousarray(img)
    h0, w0 = img.shape
    pyr = build_levels(img, levels)
    q = quotas([(L.shape[1], L.shape[0]) for L in pyr], max_points)
    pts0, desc, lev, score, bins, lxy = [], [], [], [], [], []
    for l, L in enumerate(pyr):
        xy, sc = R.top_points(*level_candidates(L, threshold), q[l])
        if not len(xy):
            continue
        d, b, status = R.describe(L, blurred(L), xy.astype(np.float32))
        assert status.all()
        h, w = L.shape
        pts0.append(np.stack([map_to_image(xy[:, 0], w0, w), map_to_image(xy[:, 1], h0, h)], axis=1))
        desc.append(d)
        lev.append(np.full(len(xy), l, np.int32))
        score.append(sc.astype(np.int32))
        bins.append(b)
        lxy.append(np.concatenate([np.full((len(xy), 1), l, np.int32), xy.astype(np.int32)], axis=1))
    if not pts0:
        return (np.empty((0, 2), np.float32), np.empty((0, 32), np.uint8), np.empty(0, np.int32), np.empty(0, np.int32), np.empty(0, np.uint8),
                np.empty((0, 3), np.int32))
    return tuple(np.concatenate(v) for v in (pts0, desc, lev, score, bins, lxy))


def keypoint_size(w0, wl):
    return np.float32(31.0 * w0 / wl)
