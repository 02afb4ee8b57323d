"""Shared inputs of the feature tests (tests/test_features_abi.py, tests/test_gpu_features.py): noise images, the hand-made FAST images, the
mosaic of oriented ramps, descriptor sets with planted neighbours, and the scene of the pipeline test with the same pipeline run
through the statement (tests/features_restate.py), the CPU oracle's blur and libvp's host RANSAC.  Everything is made once."""
import ctypes as C
import functools
import math

import numpy as np

import features_restate as R

FAST_THRESHOLD, MAX_POINTS, RATIO, MIN_MATCH, RANSAC_THRESHOLD = 20, 2000, 0.7, 10, 5.0      # what vision/utils/sift.py uses
HOMOGRAPHY = 2


def frozen(a):
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def noise(h, w, seed=0):
    return frozen(np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8))


def library(prefixes=("vp_fast_", "vp_describe_", "vp_hamming_", "vp_estimate_model_", "vp_gaussian_blur_")):
    from vision import _vp
    lib = C.CDLL(_vp.LIB_PATH)
    for name, (res, args) in _vp._SIGS.items():
        if name.startswith(prefixes) or name == "vp_last_error":
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


# ---- FAST: hand-made images ------------------------------------------------------------------------------------------------------------
def flat(h=13, w=13, v=100):
    return np.full((h, w), v, np.uint8)


def dot_image(value, v=100):
    """one pixel that differs from a flat image: all 16 ring differences are v - value"""
    img = flat(v=v)
    img[6, 6] = value
    return img


def arc_image(start, length, delta, v=100, centre=(6, 6)):
    """ring pixels start .. start + length - 1 (cyclic) of the centre are darker than it by delta, everything else is flat"""
    img = flat(v=v)
    for i in range(length):
        dx, dy = R.RING[(start + i) % 16]
        img[centre[1] + dy, centre[0] + dx] = v - delta
    return img


def twin_dots():
    """two adjacent pixels of the same value on a flat image: two corners of equal score, each the other's neighbour"""
    img = flat()
    img[6, 6] = img[6, 7] = 200
    return img


# ---- describe: oriented ramps ------------------------------------------------------------------------------------------------------------
RAMP_CELL, RAMP_COLS, RAMP_ROWS = 40, 8, 8          # 64 directions: two per bin, so that every bin is met whatever side a boundary falls


@functools.lru_cache(maxsize=None)
def ramp_mosaic():
    """(image, points): cell (r, c) holds a linear ramp that rises in direction 2 pi (8 r + c) / 64 + 0.02, its centre is the point"""
    img = np.zeros((RAMP_ROWS * RAMP_CELL, RAMP_COLS * RAMP_CELL), np.uint8)
    pts = []
    for r in range(RAMP_ROWS):
        for c in range(RAMP_COLS):
            th = 2 * math.pi * (RAMP_COLS * r + c) / (RAMP_ROWS * RAMP_COLS) + 0.02
            cy, cx = r * RAMP_CELL + RAMP_CELL // 2, c * RAMP_CELL + RAMP_CELL // 2
            yy, xx = np.mgrid[r * RAMP_CELL:(r + 1) * RAMP_CELL, c * RAMP_CELL:(c + 1) * RAMP_CELL]
            img[r * RAMP_CELL:(r + 1) * RAMP_CELL, c * RAMP_CELL:(c + 1) * RAMP_CELL] = np.clip(
                np.floor(128 + 4.0 * (math.cos(th) * (xx - cx) + math.sin(th) * (yy - cy))), 0, 255).astype(np.uint8)
            pts.append((cx, cy))
    return frozen(img), frozen(np.array(pts, np.float32))


def blurred(img):
    """B of the statement: the CPU oracle's 7 x 7 GaussianBlur at sigma 2, byte for byte the library's"""
    from oracle import oracle as orc
    return orc.gaussian_blur(np.ascontiguousarray(img), (7, 7), 2.0, 2.0)


# ---- matcher: descriptor sets --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def descriptors(n, D, seed):
    """random rows in which a few bits differ between neighbours: many equal distances, so the tie order matters"""
    r = np.random.default_rng(seed)
    base = r.integers(0, 256, (1, D), dtype=np.uint8)
    flips = (r.random((n, D * 8)) < 0.08)
    return frozen(base ^ np.packbits(flips, axis=1))


# ---- the pipeline's scene ------------------------------------------------------------------------------------------------------------
SCENE_W, SCENE_H, TEX_W, TEX_H, ANGLE, SHIFT = 240, 200, 96, 80, 10.0, (70.0, 55.0)
# The largest distance of a projected corner of the texture from its true place, in pixels, measured on stated_pipeline() (the statement,
# the oracle's blur and vp_estimate_model_host on the CPU, the committed seeds): 134 source and 382 frame keypoints, 91 matches pass
# the ratio test, all 91 are inliers.  The bound is twice that and never below 1 px: a changed default cap on the points re-draws the
# RANSAC sample.  It stays far below the RANSAC threshold of 5 px.
CORNER_ERROR_MEASURED = 0.5675683725033366
CORNER_ERROR_BOUND = max(2 * CORNER_ERROR_MEASURED, 1.0)


@functools.lru_cache(maxsize=None)
def scene():
    """(texture 80 x 96, frame 200 x 240, M 2 x 3 texture -> frame, true corners (4, 2)): a blocky random texture turned by 10 degrees
    about its centre and shifted, over a dim noisy background"""
    from oracle import oracle as orc
    r = np.random.default_rng(2024)
    # blocks of 4 x 4 softened by a 3 x 3 blur: raw axis-parallel blocks have no FAST-9 corner at all (a quadrant covers 5 ring pixels)
    tex = orc.gaussian_blur(np.kron(r.integers(0, 256, (TEX_H // 4, TEX_W // 4)), np.ones((4, 4))).astype(np.uint8), (3, 3))
    a = math.radians(ANGLE)
    cx, cy = (TEX_W - 1) / 2, (TEX_H - 1) / 2
    M = np.array([[math.cos(a), -math.sin(a), cx - math.cos(a) * cx + math.sin(a) * cy + SHIFT[0]],
                  [math.sin(a), math.cos(a), cy - math.sin(a) * cx - math.cos(a) * cy + SHIFT[1]]])
    # the texture carries value + 1 so that 0 marks "outside" after the warp; the background fills there
    body = orc.warp_affine(np.maximum(tex, 1), M, (SCENE_W, SCENE_H))
    back = r.integers(90, 110, (SCENE_H, SCENE_W)).astype(np.uint8)
    frame = np.where(body > 0, body, back).astype(np.uint8)
    corners = np.array([[0, 0], [0, TEX_H - 1], [TEX_W - 1, TEX_H - 1], [TEX_W - 1, 0]], np.float64)
    true = corners @ M[:, :2].T + M[:, 2]
    return frozen(tex), frozen(frame), frozen(M), frozen(true)


@functools.lru_cache(maxsize=None)
def unrelated_frame():
    return frozen(np.random.default_rng(77).integers(0, 256, (SCENE_H, SCENE_W), dtype=np.uint8))


def stated_detect(img):
    """(points float32 (n, 2), scores, descriptors) as SIFT._detect states them"""
    xy, score = R.top_points(*R.fast(img, FAST_THRESHOLD, True), MAX_POINTS)
    desc, _, status = R.describe(img, blurred(img), xy.astype(np.float32))
    keep = np.flatnonzero(status)
    return xy[keep].astype(np.float32), score[keep], desc[keep]


def host_ransac(src, dst):
    """(H 3 x 3 or None, mask) of libvp's host statement of the search (vp_estimate_model_host), homography, threshold 5"""
    lib = library()
    H, mask = np.zeros(9, np.float64), np.zeros(len(src), np.uint8)
    ni, nh = C.c_int(), C.c_int()
    src, dst = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(dst, np.float32)
    rc = lib.vp_estimate_model_host(src.ctypes.data, dst.ctypes.data, len(src), HOMOGRAPHY, RANSAC_THRESHOLD, 2000, 0.99, 0, H.ctypes.data, mask.ctypes.data,
                                    C.addressof(ni), C.addressof(nh))
    assert rc == 0, lib.vp_last_error(None)
    return (H.reshape(3, 3) if ni.value else None), mask


@functools.lru_cache(maxsize=None)
def stated_pipeline(which="scene"):
    """the whole of SIFT.add_source + match on the scene (or on the unrelated frame) through the statement: a dict"""
    tex, frame, _, true = scene()
    if which != "scene":
        frame = unrelated_frame()
    sp, ss, sd = stated_detect(tex)
    fp, fs, fd = stated_detect(frame)
    idx, dist = R.hamming_knn(sd, fd, 2)
    q, t = R.ratio_test(idx, dist, RATIO)
    out = {"src_pts": sp, "src_scores": ss, "src_des": sd, "pts": fp, "scores": fs, "des": fd, "idx": idx, "dist": dist, "q": q, "t": t, "H": None}
    if len(q) >= max(MIN_MATCH, 4):
        H, mask = host_ransac(sp[q], fp[t])
        out["H"], out["mask"] = H, mask
        if H is not None:
            corners = np.float32([[0, 0], [0, TEX_H - 1], [TEX_W - 1, TEX_H - 1], [TEX_W - 1, 0]])
            proj = R.perspective(H, corners)
            out["proj"], out["dst"] = proj, np.int32(proj.astype(np.float32)).reshape(4, 1, 2)
            out["corner_error"] = float(np.sqrt(((proj - true) ** 2).sum(axis=1)).max())
    return out
