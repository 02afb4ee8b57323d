"""Shared inputs of the pyramid feature tests (tests/test_pyr_features_statement.py, tests/test_pyr_features_abi.py,
tests/test_gpu_pyr_features.py): softened noise, the tiling of identical dots, and the three recognition scenes - one texture seen at
half its size, at its own size turned by 10 degrees, and at twice its size and cropped - with PyramidSIFT's pipeline run through the
statement (tests/pyr_features_restate.py), the CPU oracle's blur and libvp's host RANSAC.  Everything is made once."""
import functools
import math

import numpy as np

import features_cases as K
import features_restate as R
import pyr_features_restate as P
import resize_restate as Z

LEVELS = 8
TEX_W, TEX_H = 192, 160
SCALES = ("half", "turned", "double")
# The largest distance of a projected corner of the texture from its true place, in pixels, measured on stated_recognition() on the CPU
# with the committed seeds (1968 source keypoints; 1883 / 2000 / 2000 frame keypoints; 168 / 656 / 195 matches pass the ratio test, of
# which 161 / 652 / 191 are inliers), and the bound: twice the largest of the three.
CORNER_ERROR_MEASURED = {"half": 1.0559955243878494, "turned": 0.3205021309604006, "double": 1.9439656377879093}
CORNER_ERROR_BOUND = 2 * max(CORNER_ERROR_MEASURED.values())


@functools.lru_cache(maxsize=None)
def soft_noise(h, w, seed=0):
    """noise softened by a 3 x 3 blur, so that FAST fires on many scales"""
    from oracle import oracle as orc
    return K.frozen(orc.gaussian_blur(np.ascontiguousarray(K.noise(h, w, seed)), (3, 3)))


@functools.lru_cache(maxsize=None)
def dot_tiling(h=160, w=160, step=8, value=200, v=100):
    """a flat image with identical isolated dots `step` apart, as features_cases.dot_image makes one: every dot that can be described
    is a corner of the same score on level 0"""
    img = np.full((h, w), v, np.uint8)
    img[4::step, 4::step] = value
    return K.frozen(img)


@functools.lru_cache(maxsize=None)
def texture(seed=2024):
    from oracle import oracle as orc
    r = np.random.default_rng(seed)
    return K.frozen(orc.gaussian_blur(np.kron(r.integers(0, 256, (TEX_H // 4, TEX_W // 4)), np.ones((4, 4))).astype(np.uint8), (3, 3)))


def _paste(frame_w, frame_h, body, ox, oy, seed):
    """body (value 0 = outside) at (ox, oy) over a dim noisy background, cropped to the frame"""
    back = np.random.default_rng(seed).integers(90, 110, (frame_h, frame_w)).astype(np.uint8)
    bh, bw = body.shape
    x0, y0, x1, y1 = max(ox, 0), max(oy, 0), min(ox + bw, frame_w), min(oy + bh, frame_h)
    part = body[y0 - oy:y1 - oy, x0 - ox:x1 - ox]
    back[y0:y1, x0:x1] = np.where(part > 0, part, back[y0:y1, x0:x1])
    return back


SOURCE_CORNERS = np.array([[0, 0], [0, TEX_H - 1], [TEX_W - 1, TEX_H - 1], [TEX_W - 1, 0]], np.float64)


@functools.lru_cache(maxsize=None)
def scene(which):
    """(frame, true corners (4, 2) of the texture in the frame)"""
    from oracle import oracle as orc
    tex = np.maximum(texture(), 1)                       # 0 marks "outside"
    if which == "half":
        ox, oy = 70, 55
        small = Z.resize(tex, (TEX_W // 2, TEX_H // 2))
        return K.frozen(_paste(240, 200, small, ox, oy, 11)), K.frozen((SOURCE_CORNERS + 0.5) * 0.5 - 0.5 + [ox, oy])
    if which == "double":
        ox, oy = 20, 15
        big = Z.resize(tex, (TEX_W * 2, TEX_H * 2))
        return K.frozen(_paste(320, 260, big, ox, oy, 12)), K.frozen((SOURCE_CORNERS + 0.5) * 2.0 - 0.5 + [ox, oy])
    assert which == "turned"
    a = math.radians(K.ANGLE)
    cx, cy = (TEX_W - 1) / 2, (TEX_H - 1) / 2
    sx, sy = 60.0, 48.0
    M = np.array([[math.cos(a), -math.sin(a), cx - math.cos(a) * cx + math.sin(a) * cy + sx],
                  [math.sin(a), math.cos(a), cy - math.sin(a) * cx - math.cos(a) * cy + sy]])
    body = orc.warp_affine(tex, M, (320, 260))
    return K.frozen(_paste(320, 260, body, 0, 0, 13)), K.frozen(SOURCE_CORNERS @ M[:, :2].T + M[:, 2])


@functools.lru_cache(maxsize=None)
def stated_features(key):
    """the statement's pyramid_features of the texture ("source") or of a scene, with PyramidSIFT's parameters"""
    img = texture() if key == "source" else scene(key)[0]
    return P.pyramid_features(img, K.FAST_THRESHOLD, K.MAX_POINTS, LEVELS)


@functools.lru_cache(maxsize=None)
def stated_recognition(which):
    """the whole of PyramidSIFT.add_source + match on one scene through the statement: a dict"""
    sp, sd = stated_features("source")[:2]
    fp, fd = stated_features(which)[:2]
    idx, dist = R.hamming_knn(sd, fd, 2)
    q, t = R.ratio_test(idx, dist, K.RATIO)
    out = {"idx": idx, "dist": dist, "q": q, "t": t, "H": None, "inliers": 0}
    if len(q) >= max(K.MIN_MATCH, 4):
        H, mask = K.host_ransac(sp[q], fp[t])
        out["H"], out["mask"] = H, mask
        if H is not None:
            proj = R.perspective(H, np.float32(SOURCE_CORNERS))
            out["proj"], out["dst"] = proj, np.int32(proj.astype(np.float32)).reshape(4, 1, 2)
            out["inliers"] = int(mask.sum())
            out["corner_error"] = float(np.sqrt(((proj - scene(which)[1]) ** 2).sum(axis=1)).max())
    return out
