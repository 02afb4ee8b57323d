"""Cases and comparison helpers of the colour-balance tests (tests/test_balance_cases.py, tests/test_gpu_balance.py and its child
tests/_balance_fold_worker.py), in one place so that the parent and the child test the same things.  Every expectation comes from
`oracle.color_balance(..., mean_mode=0)`: the reference's running tile mean (cpp:452-467), literally."""
import ctypes as C

import numpy as np

import frames as F

# (h, w): tilings (hb, vb).  Together: bw % 4 != 0 (15, 5, 9, 3, 1), w % 4 != 0 (30, 45, 9), npx % 4 != 0 (21 x 45, 7 x 9), tiles in the
# last row and the last column, bh == bw == 1 ((9, 7) on 7 x 9: one-pixel tiles), and four-pixel groups that straddle a tile edge and
# a row end.
TILED_CASES = [
    ((20, 30), [(2, 4), (6, 5)]),
    ((21, 45), [(3, 7), (9, 3), (5, 1)]),
    ((24, 32), [(2, 2), (8, 1)]),
    ((7, 9), [(3, 1), (9, 7)]),
]
NOT_DIVIDING = {(20, 30): (4, 3), (21, 45): (4, 2), (24, 32): (5, 7), (7, 9): (2, 2)}   # (h, w): a tiling (hb, vb) that divides neither side
SMALL_FRAMES = [(1, 1), (1, 7), (7, 1), (2, 2)]                                          # (h, w)
BASE_BGR =(124.0, 128.0, 134.0)   # channels close together: which of them leads (the cast, cpp:476-541) changes from tile to tile
CAST = 0.08                        # each tile's channel means move by up to +-8 %: inside the 1/6 band of cpp:474 with the noise on top
NOISE = 3                          # +-3 grey levels


def tiled_frame(h, w, hb, vb, seed):
    """A BGR frame whose (hb x vb) tiles each carry their own cast: base colour, every tile's three channel means moved by their own
    amounts (at most CAST, so that the 1/6 rule keeps the tile's means), plus small noise."""
    assert w % hb == 0 and h % vb == 0, (h, w, hb, vb)
    rng = np.random.default_rng(seed)
    bw, bh = w // hb, h // vb
    shift = rng.uniform(-CAST, CAST, (vb, hb, 3))
    means = np.rint(np.asarray(BASE_BGR) * (1.0 + shift))                         # (vb, hb, 3)
    img = np.repeat(np.repeat(means, bh, axis=0), bw, axis=1)                      # (h, w, 3)
    img = img + rng.integers(-NOISE, NOISE + 1, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def tiled_cases():
    """[(name, frame, hb, vb)]: every frame / tiling of TILED_CASES, the frame built for that tiling."""
    out = []
    for k, ((h, w), tilings) in enumerate(TILED_CASES):
        for j, (hb, vb) in enumerate(tilings):
            out.append(("%dx%d tiles %dx%d" % (h, w, hb, vb), tiled_frame(h, w, hb, vb, 100 * k + j), hb, vb))
    return out


def tile_index(h, w, hb, vb):
    """(h, w) array: the tile (row-major, by * hb + bx) every pixel belongs to."""
    yy, xx = np.mgrid[0:h, 0:w]
    return (yy // (h // vb)) * hb + xx // (w // hb)


def batch_frames():
    """Three different 30 x 40 frames (h x w; npx * 3 % 4 == 0, as the batched entry wants): buoy, bins, noise."""
    return np.stack([F.s1_buoy(1, 40, 30), F.s2_bins(2, 40, 30), F.s3_noise(3, 40, 30)])


BATCH_TILINGS = [(1, 1), (2, 2), (8, 5)]


def flag_bits(vp, equalize_rgb=True, rgb_contrast_correct=False, hsv_contrast_correct=True, hsi_contrast_correct=False,
              rgb_extrema_clipping=True, adaptive_cast_correction=False):
    """The VP_CB_* word of balance()'s keyword arguments, for the C ABI."""
    return ((vp.CB_EQUALIZE_RGB if equalize_rgb else 0) | (vp.CB_RGB_CONTRAST if rgb_contrast_correct else 0) |
            (vp.CB_HSV_CONTRAST if hsv_contrast_correct else 0) | (vp.CB_HSI_CONTRAST if hsi_contrast_correct else 0) |
            (vp.CB_EXTREMA_CLIPPING if rgb_extrema_clipping else 0) | (vp.CB_ADAPTIVE_CAST if adaptive_cast_correction else 0))


GUARD = 64
FILL = 0xA5


def run_dev(vp, frames, flags, hb, vb, in_place):
    """vp_color_balance_dev on (n, h, w, 3) frames.  The destination is pre-filled with FILL and followed by GUARD bytes of FILL.
    -> (rc, dst bytes as frames, src bytes read back, guard bytes); the buffers are synchronised and freed whatever rc is."""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    n, h, w, _ = frames.shape
    ctx, L = vp.default_context(), vp.lib()
    nb = frames.nbytes
    d_src, d_dst = C.c_void_p(), C.c_void_p()
    fill = np.full(nb + GUARD, FILL, np.uint8)
    vp.check(L.vp_dev_alloc(ctx.handle, nb + GUARD, C.byref(d_dst)), ctx.handle)
    vp.check(L.vp_memcpy_h2d(ctx.handle, d_dst, vp.ptr(fill), nb + GUARD), ctx.handle)
    if in_place:
        d_src = d_dst
    else:
        vp.check(L.vp_dev_alloc(ctx.handle, nb, C.byref(d_src)), ctx.handle)
    vp.check(L.vp_memcpy_h2d(ctx.handle, d_src, vp.ptr(frames), nb), ctx.handle)
    rc = L.vp_color_balance_dev(ctx.handle, d_src, d_dst, w, h, n, int(flags), int(hb), int(vb))
    ctx.synchronize()
    out = np.empty(nb + GUARD, np.uint8)
    back = np.empty(nb, np.uint8)
    vp.check(L.vp_memcpy_d2h(ctx.handle, vp.ptr(out), d_dst, nb + GUARD), ctx.handle)
    vp.check(L.vp_memcpy_d2h(ctx.handle, vp.ptr(back), d_src, nb), ctx.handle)
    vp.check(L.vp_dev_free(ctx.handle, d_dst), ctx.handle)
    if not in_place:
        vp.check(L.vp_dev_free(ctx.handle, d_src), ctx.handle)
    return rc, out[:nb].reshape(frames.shape), back.reshape(frames.shape), out[nb:]


def last_folds(vp):
    ctx = vp.default_context()
    n = C.c_int32(-1)
    vp.check(vp.lib().vp_color_balance_last_folds(ctx.handle, C.byref(n)), ctx.handle)
    return n.value


def assert_exact(got, exp, what):
    assert got.shape == exp.shape and got.dtype == np.uint8, (what, got.shape, got.dtype)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, (what, "%d values differ, first at %s: got %d, expected %d"
                           % (len(bad), bad[0].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])]))


def assert_hsi(got, exp, what):
    """The tolerance tests/test_gpu_balance.py states for the HSI stage: at most 1, on fewer than 5e-3 of the values."""
    d = np.abs(got.astype(int) - exp.astype(int))
    assert d.max() <= 1, (what, int(d.max()))
    assert (d > 0).mean() < 5e-3, (what, float((d > 0).mean()))
