"""The statement of cv2.equalizeHist and cv2.createCLAHE(clipLimit, tileGridSize).apply on 8-bit single-channel images, twice: once
following OpenCV's loops literally (`*_loops`), once as vectorised closed forms (`equalize_hist`, `clahe`).  The two share nothing
but numpy and are checked against each other by tests/test_clahe_statement.py; the GPU suite compares the kernels with the
vectorised form.  All float arithmetic is numpy float32: every product and every sum is rounded on its own (nothing is fused),
np.rint rounds ties to even as cvRound does.

The geometry quirk that is part of the contract: when EITHER w % tilesX or h % tilesY is non-zero, the image is extended on the right
by tilesX - w % tilesX AND at the bottom by tilesY - h % tilesY (BORDER_REFLECT_101), so a dimension that does divide grows by a
whole tilesX / tilesY."""
import numpy as np

F = np.float32


def _u8(v):
    """saturate_cast<uchar>(cvRound(v)) of float32 values"""
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


# ---- geometry and clip limit (shared: plain integer statements of the issue, no image arithmetic) ------------------------------------
def geometry(w, h, tiles_x, tiles_y):
    """(ext_w, ext_h, tile_w, tile_h)"""
    if w % tiles_x == 0 and h % tiles_y == 0:
        ew, eh = w, h
    else:
        ew, eh = w + tiles_x - w % tiles_x, h + tiles_y - h % tiles_y
    return ew, eh, ew // tiles_x, eh // tiles_y


def clip_count(clip_limit, area):
    """the integer clip limit per bin: 0 = no clipping; double arithmetic truncated, at least 1"""
    if clip_limit <= 0:
        return 0
    return max(int(float(clip_limit) * area / 256), 1)


def supported(w, h, clip_limit, tiles_x, tiles_y):
    """what the library accepts without VP_ERR_UNSUPPORTED / VP_ERR_INVALID"""
    if w <= 0 or h <= 0 or tiles_x < 1 or tiles_y < 1 or clip_limit != clip_limit:
        return False
    if tiles_x > 64 or tiles_y > 64 or w * h > 1 << 28:
        return False
    ew, eh, tw, th = geometry(w, h, tiles_x, tiles_y)
    if ew != w and (ew - w >= w or eh - h >= h):       # padded: single reflection only
        return False
    return not (clip_limit > 0 and float(clip_limit) * (tw * th) / 256 >= 2.0 ** 31)


def reflect101(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101) for p >= 0 after a single reflection"""
    return p if p < n else 2 * n - 2 - p


# ---- equalizeHist ----------------------------------------------------------------------------------------------------------------------
def equalize_hist_loops(src):
    src = np.asarray(src)
    h, w = src.shape
    hist = [0] * 256
    for y in range(h):
        for x in range(w):
            hist[int(src[y, x])] += 1
    total = w * h
    i = 0
    while hist[i] == 0:
        i += 1
    if hist[i] == total:
        return np.full((h, w), i, np.uint8)
    scale = F(255) / F(total - hist[i])
    lut = [0] * 256
    s = 0
    for j in range(i + 1, 256):
        s += hist[j]
        lut[j] = int(_u8(F(s) * scale))
    out = np.empty((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            out[y, x] = lut[int(src[y, x])]
    return out


def equalize_hist(src):
    src = np.asarray(src)
    hist = np.bincount(src.ravel(), minlength=256).astype(np.int64)
    i0 = int(np.flatnonzero(hist)[0])
    if hist[i0] == src.size:
        return np.full(src.shape, i0, np.uint8)
    scale = F(255) / F(src.size - hist[i0])
    above = np.where(np.arange(256) > i0, hist, 0)
    lut = _u8(np.cumsum(above).astype(F) * scale)
    lut[:i0 + 1] = 0
    return lut[src]


# ---- CLAHE: the residual's distribution ----------------------------------------------------------------------------------------------------
def residual_bins_loop(residual):
    """bins that get +1 from the literal loop `for (i = 0; i < 256 && residual > 0; i += step, residual--)`; and whether it ran out of bins"""
    step = max(256 // residual, 1)
    bins = []
    i = 0
    while i < 256 and residual > 0:
        bins.append(i)
        i += step
        residual -= 1
    return bins, residual > 0


def residual_bins_closed(residual):
    step = max(256 // residual, 1)
    return [i for i in range(256) if i % step == 0 and i // step < residual]


# ---- CLAHE, literal loops ----------------------------------------------------------------------------------------------------------------
def tile_lut_loops(pixels, clip, area):
    """pixels: the tile's `area` bytes; the 256-entry table"""
    hist = [0] * 256
    for v in pixels:
        hist[int(v)] += 1
    if clip > 0:
        clipped = 0
        for i in range(256):
            if hist[i] > clip:
                clipped += hist[i] - clip
                hist[i] = clip
        batch = clipped // 256
        residual = clipped - batch * 256
        for i in range(256):
            hist[i] += batch
        if residual != 0:
            step = max(256 // residual, 1)
            i = 0
            while i < 256 and residual > 0:
                hist[i] += 1
                i += step
                residual -= 1
    scale = F(255) / F(area)
    sums = []
    s = 0
    for i in range(256):
        s += hist[i]
        sums.append(s)
    return _u8(np.array(sums, np.int64).astype(F) * scale)    # per bin: saturate_cast<uchar>(float32(sum) * scale), one multiply each


def clahe_loops(src, clip_limit, tile_grid):
    src = np.asarray(src)
    h, w = src.shape
    tiles_x, tiles_y = int(tile_grid[0]), int(tile_grid[1])
    ew, eh, tw, th = geometry(w, h, tiles_x, tiles_y)
    area = tw * th
    clip = clip_count(clip_limit, area)
    luts = np.empty((tiles_y, tiles_x, 256), np.uint8)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            px = [src[reflect101(y, h), reflect101(x, w)] for y in range(ty * th, ty * th + th) for x in range(tx * tw, tx * tw + tw)]
            luts[ty, tx] = tile_lut_loops(px, clip, area)
    inv_tw, inv_th = F(1) / F(tw), F(1) / F(th)
    out = np.empty((h, w), np.uint8)
    for y in range(h):
        tyf = F(y) * inv_th - F(0.5)
        ty1 = int(np.floor(tyf))
        ya = tyf - F(ty1)
        ya1 = F(1) - ya
        ty2 = min(ty1 + 1, tiles_y - 1)
        ty1 = max(ty1, 0)
        for x in range(w):
            txf = F(x) * inv_tw - F(0.5)
            tx1 = int(np.floor(txf))
            xa = txf - F(tx1)
            xa1 = F(1) - xa
            tx2 = min(tx1 + 1, tiles_x - 1)
            tx1 = max(tx1, 0)
            v = int(src[y, x])
            res = (F(luts[ty1, tx1, v]) * xa1 + F(luts[ty1, tx2, v]) * xa) * ya1 + (F(luts[ty2, tx1, v]) * xa1 + F(luts[ty2, tx2, v]) * xa) * ya
            out[y, x] = _u8(res)
    return out


# ---- CLAHE, vectorised -----------------------------------------------------------------------------------------------------------------------
def tile_luts(src, clip_limit, tile_grid):
    """(tiles_y, tiles_x, 256) uint8 tables"""
    src = np.asarray(src)
    h, w = src.shape
    tiles_x, tiles_y = int(tile_grid[0]), int(tile_grid[1])
    ew, eh, tw, th = geometry(w, h, tiles_x, tiles_y)
    area = tw * th
    ys, xs = np.arange(eh), np.arange(ew)
    ext = src[np.where(ys < h, ys, 2 * h - 2 - ys)][:, np.where(xs < w, xs, 2 * w - 2 - xs)]
    tiles = ext.reshape(tiles_y, th, tiles_x, tw).transpose(0, 2, 1, 3).reshape(tiles_y * tiles_x, area).astype(np.int64)
    hist = np.zeros((tiles_y * tiles_x, 256), np.int64)
    np.add.at(hist, (np.repeat(np.arange(len(tiles)), area), tiles.ravel()), 1)
    clip = clip_count(clip_limit, area)
    if clip > 0:
        clipped = np.maximum(hist - clip, 0).sum(axis=1)
        hist = np.minimum(hist, clip)
        batch, residual = clipped // 256, clipped % 256
        step = np.maximum(256 // np.maximum(residual, 1), 1)
        i = np.arange(256)[None, :]
        extra = (residual[:, None] != 0) & (i % step[:, None] == 0) & (i // step[:, None] < residual[:, None])
        hist = hist + batch[:, None] + extra
    scale = F(255) / F(area)
    return _u8(np.cumsum(hist, axis=1).astype(F) * scale).reshape(tiles_y, tiles_x, 256)


def _axis(n, tile, tiles):
    """per coordinate: clamped tile indices and the float32 weights, computed before the clamps"""
    f = np.arange(n).astype(F) * (F(1) / F(tile)) - F(0.5)
    lo = np.floor(f).astype(np.int64)
    a = f - lo.astype(F)
    return np.maximum(lo, 0), np.minimum(lo + 1, tiles - 1), a.astype(F), (F(1) - a).astype(F)


def clahe(src, clip_limit=40.0, tile_grid=(8, 8)):
    src = np.asarray(src)
    h, w = src.shape
    tiles_x, tiles_y = int(tile_grid[0]), int(tile_grid[1])
    _, _, tw, th = geometry(w, h, tiles_x, tiles_y)
    luts = tile_luts(src, clip_limit, tile_grid).astype(F)
    tx1, tx2, xa, xa1 = _axis(w, tw, tiles_x)
    ty1, ty2, ya, ya1 = _axis(h, th, tiles_y)
    v = src.astype(np.int64)
    Y1, Y2, X1, X2 = ty1[:, None], ty2[:, None], tx1[None, :], tx2[None, :]
    xa, xa1, ya, ya1 = xa[None, :], xa1[None, :], ya[:, None], ya1[:, None]
    top = luts[Y1, X1, v] * xa1 + luts[Y1, X2, v] * xa
    bot = luts[Y2, X1, v] * xa1 + luts[Y2, X2, v] * xa
    res = top * ya1 + bot * ya
    assert res.dtype == F
    return _u8(res)


def clahe_fused_f64(src, clip_limit=40.0, tile_grid=(8, 8)):
    """The blend as a compiler that contracts a * b + c into fused multiply-adds would evaluate it (open points):
    fma(a, b, c) is emulated as float32(float64(a) * float64(b) + float64(c)): the float64 product of two float32 values is exact, and
    the float64 sum is off from the exact one by at most 2^-53 relative, far below what decides a float32 rounding in all but
    vanishingly rare cases - good for a count, not for a contract."""
    src = np.asarray(src)
    h, w = src.shape
    tiles_x, tiles_y = int(tile_grid[0]), int(tile_grid[1])
    _, _, tw, th = geometry(w, h, tiles_x, tiles_y)
    luts = tile_luts(src, clip_limit, tile_grid).astype(np.float64)
    tx1, tx2, xa, xa1 = _axis(w, tw, tiles_x)
    ty1, ty2, ya, ya1 = _axis(h, th, tiles_y)
    v = src.astype(np.int64)
    Y1, Y2, X1, X2 = ty1[:, None], ty2[:, None], tx1[None, :], tx2[None, :]
    xa, xa1, ya, ya1 = (a.astype(np.float64) for a in (xa[None, :], xa1[None, :], ya[:, None], ya1[:, None]))

    def fma(a, b, c):
        return (a * b + c).astype(F).astype(np.float64)

    def mul(a, b):
        return (a * b).astype(F).astype(np.float64)
    top = fma(luts[Y1, X1, v], xa1, mul(luts[Y1, X2, v], xa))
    bot = fma(luts[Y2, X1, v], xa1, mul(luts[Y2, X2, v], xa))
    return _u8(fma(top, ya1, mul(bot, ya)).astype(F))
