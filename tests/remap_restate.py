"""cv2.remap, cv2.convertMaps and cv2.warpPerspective on 8-bit images restated in numpy from DESIGN.md section 4.21 (OpenCV's
classical fixed-point path, releases up to 4.10).  Test infrastructure only: it never calls the library under test.

Every source coordinate becomes an int16 integer part and a fraction index fy * 32 + fx (five bits each); a linear sample blends
the four neighbours with the weights (32 - fx)(32 - fy) 32, fx (32 - fy) 32, (32 - fx) fy 32, fx fy 32 and rounds
(sum + 2^14) >> 15; a nearest sample reads one pixel.  BORDER_CONSTANT substitutes the border value per neighbour (four outside
neighbours therefore give the border value itself), BORDER_REPLICATE clamps each neighbour's coordinates.  float32 and float64
arithmetic is numpy's element-wise IEEE arithmetic: one rounding per operation, no fused multiply-add."""
import numpy as np

INT_MIN, INT_MAX = -2147483648, 2147483647


def cv_round_f32(v):
    """cvRound(float): round half to even; outside int32 (and NaN) x86 gives INT_MIN, which nothing promises"""
    v = np.asarray(v, np.float32)
    ok = (v >= np.float32(-2147483648.0)) & (v < np.float32(2147483648.0))
    return np.where(ok, np.rint(np.where(ok, v, 0)).astype(np.int64), INT_MIN)


def sat16(v):
    return np.clip(v, -32768, 32767)


def convert_maps_restate(mapx, mapy=None, nearest=False):
    """float32 maps (two planes, or one (h, w, 2) plane) -> (int16 (h, w, 2), uint16 (h, w) fraction indices; None for nearest)"""
    mapx = np.asarray(mapx, np.float32)
    if mapy is None:
        mapx, mapy = mapx[:, :, 0], mapx[:, :, 1]
    mapy = np.asarray(mapy, np.float32)
    if nearest:
        return np.stack([sat16(cv_round_f32(mapx)), sat16(cv_round_f32(mapy))], axis=-1).astype(np.int16), None
    ix = cv_round_f32(mapx * np.float32(32))
    iy = cv_round_f32(mapy * np.float32(32))
    xy = np.stack([sat16(ix >> 5), sat16(iy >> 5)], axis=-1).astype(np.int16)
    return xy, ((iy & 31) * 32 + (ix & 31)).astype(np.uint16)


def _border_value(value, cn):
    v = np.zeros(4, np.int64)
    vals = np.atleast_1d(np.asarray(value)).ravel()[:4]
    v[:len(vals)] = vals
    return v[:cn]


def sample_restate(src, sx, sy, frac, nearest, border, value):
    """src (h, w) or (h, w, cn) uint8; sx, sy integer parts and frac fraction indices, all of the destination's (dh, dw) shape"""
    src = np.asarray(src)
    img = (src if src.ndim == 3 else src[:, :, None]).astype(np.int64)
    sh, sw, cn = img.shape
    cval = _border_value(value, cn)
    sx, sy = np.asarray(sx, np.int64), np.asarray(sy, np.int64)

    def tap(x, y):
        inside = (x >= 0) & (x < sw) & (y >= 0) & (y < sh)
        px = img[np.clip(y, 0, sh - 1), np.clip(x, 0, sw - 1)]
        if border == "replicate":
            return px
        assert border == "constant"
        return np.where(inside[..., None], px, cval)
    if nearest:
        out = tap(sx, sy)
    else:
        frac = np.asarray(frac, np.int64)
        fx, fy = (frac & 31)[..., None], ((frac >> 5) & 31)[..., None]
        acc = tap(sx, sy) * ((32 - fx) * (32 - fy) * 32) + tap(sx + 1, sy) * (fx * (32 - fy) * 32) + \
            tap(sx, sy + 1) * ((32 - fx) * fy * 32) + tap(sx + 1, sy + 1) * (fx * fy * 32)
        out = (acc + (1 << 14)) >> 15
    out = np.clip(out, 0, 255).astype(np.uint8)
    return out if src.ndim == 3 else out[:, :, 0]


def remap_restate(src, map1, map2=None, nearest=False, border="constant", value=0):
    """cv2.remap(src, map1, map2, INTER_NEAREST if nearest else INTER_LINEAR, borderMode, borderValue): float maps are converted as
    convertMaps converts them; the fixed form is used as it is (the low ten bits of the fraction plane)"""
    map1 = np.asarray(map1)
    if map1.dtype == np.int16:
        xy, frac = map1, (None if map2 is None else np.asarray(map2).reshape(map1.shape[:2]).astype(np.int64) & 1023)
        assert (frac is None) == bool(nearest)
    else:
        xy, frac = convert_maps_restate(map1, map2, nearest)
    return sample_restate(src, xy[:, :, 0], xy[:, :, 1], frac, nearest, border, value)


def invert33_restate(M):
    """cv::invert of a 3x3 double matrix: determinant by cofactors, d = 1 / det, every cofactor times d; zeros when det == 0"""
    S = [[float(v) for v in row] for row in np.asarray(M, np.float64)]
    d = S[0][0] * (S[1][1] * S[2][2] - S[1][2] * S[2][1]) - S[0][1] * (S[1][0] * S[2][2] - S[1][2] * S[2][0]) + S[0][2] * (S[1][0] * S[2][1] - S[1][1] * S[2][0])
    if d == 0.0:
        return np.zeros((3, 3))
    d = 1.0 / d
    return np.array([[(S[1][1] * S[2][2] - S[1][2] * S[2][1]) * d, (S[0][2] * S[2][1] - S[0][1] * S[2][2]) * d, (S[0][1] * S[1][2] - S[0][2] * S[1][1]) * d],
                     [(S[1][2] * S[2][0] - S[1][0] * S[2][2]) * d, (S[0][0] * S[2][2] - S[0][2] * S[2][0]) * d, (S[0][2] * S[1][0] - S[0][0] * S[1][2]) * d],
                     [(S[1][0] * S[2][1] - S[1][1] * S[2][0]) * d, (S[0][1] * S[2][0] - S[0][0] * S[2][1]) * d, (S[0][0] * S[1][1] - S[0][1] * S[1][0]) * d]])


def block_width(dw, dh):
    bh0 = min(16, dh)
    return min(1024 // bh0, dw)


def _clamp_round(v):
    """saturate_cast<int>(std::max((double)INT_MIN, std::min((double)INT_MAX, v))) with std::min / std::max's operand order"""
    t = np.where(v < float(INT_MAX), v, float(INT_MAX))
    t = np.where(float(INT_MIN) < t, t, float(INT_MIN))
    return np.rint(t).astype(np.int64)


def warp_perspective_coords(M, dsize, inverse_map=False, nearest=False):
    """(sx, sy, frac) of every destination pixel, block-origin form: X0 = M0 bx + M1 y + M2 per block, then X0 + M0 (x - bx)"""
    dw, dh = dsize
    m = (np.asarray(M, np.float64) if inverse_map else invert33_restate(M)).ravel()
    bw0 = block_width(dw, dh)
    x = np.arange(dw, dtype=np.int64)[None, :]
    y = np.arange(dh, dtype=np.float64)[:, None]
    bx = ((x // bw0) * bw0).astype(np.float64)
    x1 = x.astype(np.float64) - bx
    X0 = (m[0] * bx + m[1] * y) + m[2]
    Y0 = (m[3] * bx + m[4] * y) + m[5]
    W0 = (m[6] * bx + m[7] * y) + m[8]
    W = W0 + m[6] * x1
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        W = np.where(W != 0, (1.0 if nearest else 32.0) / np.where(W != 0, W, 1.0), 0.0)
        X = _clamp_round((X0 + m[0] * x1) * W)
        Y = _clamp_round((Y0 + m[3] * x1) * W)
    if nearest:
        return sat16(X), sat16(Y), None
    return sat16(X >> 5), sat16(Y >> 5), (Y & 31) * 32 + (X & 31)


def warp_perspective_restate(src, M, dsize, inverse_map=False, nearest=False, border="constant", value=0):
    """cv2.warpPerspective(src, M, dsize, flags, borderMode, borderValue); dsize = (width, height)"""
    sx, sy, frac = warp_perspective_coords(M, dsize, inverse_map, nearest)
    return sample_restate(src, sx, sy, frac, nearest, border, value)
