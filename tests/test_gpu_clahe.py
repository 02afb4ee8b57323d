"""GPU suite for cv2.equalizeHist and CLAHE (vp_equalize_hist_*, vp_clahe_*, vision.utils.color.equalize_hist / clahe / clahe_bgr,
cv2_facade.equalizeHist / createCLAHE).

Every comparison is byte for byte.  Expectations come from the vectorised form of tests/clahe_restate.py (checked against its
literal-loop form on the CPU by tests/test_clahe_statement.py), never from the library under test.  The shapes are the smallest at
which each path of the kernels is taken: tiles cut from the image and from its reflected extension, the whole-tile padding quirk,
tiles that lie wholly in the extension (9 x 9 on 8 x 8), clamped neighbours, one block per tile and several, rows that keep dword
stores aligned and rows that do not, tables staged in LDS and (from 257 tiles on) read from device memory."""
import functools

import numpy as np
import pytest

import clahe_restate as R

pytestmark = pytest.mark.gpu

CLIPS = [0, 1e-3, 2.0, 40.0, 1e4]
# (w, h), (tiles_x, tiles_y)
CASES = [((64, 64), (8, 8)), ((16, 16), (8, 8)), ((37, 29), (4, 3)), ((40, 29), (4, 3)), ((9, 9), (8, 8)), ((61, 45), (1, 1)), ((61, 45), (1, 8)), ((61, 45), (8, 1)),
         ((256, 192), (2, 2))]


@functools.lru_cache(maxsize=None)
def _image(w, h, kind="random"):
    rng = np.random.default_rng(w * 1009 + h)
    if kind == "random":
        a = rng.integers(0, 256, (h, w), dtype=np.uint8)
    elif kind == "narrow":                              # a few grey levels: clipping cuts a lot, the residual matters
        a = rng.integers(90, 99, (h, w), dtype=np.uint8)
    else:
        a = np.full((h, w), 131, np.uint8)
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def _expect(w, h, kind, clip, grid):
    out = R.clahe(_image(w, h, kind), clip, grid)
    out.flags.writeable = False
    return out


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _dev(ctx, arr):
    from vision.devmat import DeviceMat
    return DeviceMat.from_host(ctx, np.ascontiguousarray(arr))


def _check(ctx, w, h, kind, clip, grid):
    """vision.utils.color.clahe with a numpy source (the host entry) and a DeviceMat source (the device entry) against the statement"""
    from vision.devmat import DeviceMat
    from vision.utils import color
    img, exp = _image(w, h, kind), _expect(w, h, kind, clip, grid)
    host = color.clahe(img, clip, grid)
    assert type(host) is np.ndarray and _same(host, exp), (w, h, kind, clip, grid, "host entry", int((host != exp).sum()))
    src = _dev(ctx, img)
    out = color.clahe(src, clip, grid)
    assert isinstance(out, DeviceMat) and out.dtype == np.uint8 and out.shape == (h, w) and out.binary is False
    assert out._host is None and src._host is None, "a host copy was made"
    got = np.asarray(out)
    assert _same(got, exp), (w, h, kind, clip, grid, "device entry", int((got != exp).sum()))


@pytest.mark.parametrize("size,grid", CASES)
def test_clahe_equals_the_statement_at_every_clip_limit(vp, size, grid):
    ctx = vp.default_context()
    for clip in CLIPS:
        for kind in ("random", "narrow", "constant"):
            _check(ctx, size[0], size[1], kind, clip, grid)


@pytest.mark.parametrize("split", [1, 2, 5, 64])
def test_forced_split_gives_identical_bytes(vp, split):
    """256 x 192 on (2, 2): tiles of 128 x 96.  One block per tile, and 2, 5 (ragged: 20 rows each, the last block 16) and 64 blocks
    that add partial histograms with device atomics, against the statement and so against each other; the padded 37 x 29 as well."""
    ctx = vp.default_context()
    try:
        ctx.set_option(vp.OPT_CLAHE_SPLIT, split)
        for clip in (0, 2.0, 40.0):
            _check(ctx, 256, 192, "random", clip, (2, 2))
            _check(ctx, 256, 192, "narrow", clip, (2, 2))
        _check(ctx, 37, 29, "random", 2.0, (4, 3))
        _check(ctx, 9, 9, "random", 40.0, (8, 8))
    finally:
        ctx.set_option(vp.OPT_CLAHE_SPLIT, 0)
    for bad in (-1, 65):
        with pytest.raises(vp.VpError):
            ctx.set_option(vp.OPT_CLAHE_SPLIT, bad)


def test_more_tiles_than_the_lds_budget_holds_read_their_tables_from_device_memory(vp):
    """(17, 16) = 272 tiles of 256 bytes is above the 64 KiB the interpolation kernel stages; (16, 16) fills it exactly"""
    ctx = vp.default_context()
    _check(ctx, 85, 64, "random", 2.0, (17, 16))
    _check(ctx, 80, 64, "random", 2.0, (16, 16))
    _check(ctx, 130, 67, "random", 40.0, (64, 64))


def test_strided_source_at_an_odd_offset_with_a_width_that_is_no_multiple_of_four(vp):
    """A column window of a wider device image through the C ABI: the first byte at an odd address, a stride that is no multiple of 4,
    so every row starts at another phase; widths 4 k + 1, 2, 3 take the byte stores, 4 k the dword stores."""
    from vision.devmat import DeviceMat
    ctx = vp.default_context()
    L = vp.lib()
    rng = np.random.default_rng(9)
    H, x0 = 45, 31
    for W, w in ((201, 67), (203, 66), (333, 65), (200, 68), (131, 100)):
        wide = rng.integers(0, 256, (H, W), dtype=np.uint8)
        win = np.ascontiguousarray(wide[:, x0:x0 + w])
        buf = _dev(ctx, wide)
        assert (buf.dev_ptr + x0) % 2 == 1
        for clip, grid in ((2.0, (4, 3)), (40.0, (8, 8)), (0, (1, 1))):
            out = DeviceMat(ctx, (H, w))
            vp.check(L.vp_clahe_dev(ctx.handle, buf.dev_ptr + x0, W, w, H, clip, grid[0], grid[1], out.dev_ptr), ctx.handle)
            assert _same(np.asarray(out), R.clahe(win, clip, grid)), (W, w, clip, grid)
        out = DeviceMat(ctx, (H, w))
        vp.check(L.vp_equalize_hist_dev(ctx.handle, buf.dev_ptr + x0, W, w, H, out.dev_ptr), ctx.handle)
        assert _same(np.asarray(out), R.equalize_hist(win)), (W, w)


def test_full_size_frame_at_the_default_grid(vp):
    import frames as F
    from vision import cv2_facade as f
    ctx = vp.default_context()
    grey = np.ascontiguousarray(F.s1_buoy(0, 1920, 1080)[:, :, 1])
    exp = R.clahe(grey, 40.0, (8, 8))
    src = _dev(ctx, grey)
    out = f.createCLAHE().apply(src)                      # cv2's defaults: clipLimit 40, (8, 8)
    assert _same(np.asarray(out), exp)
    out2 = f.createCLAHE(2.0).apply(src)
    assert _same(np.asarray(out2), R.clahe(grey, 2.0, (8, 8)))
    assert _same(np.asarray(f.equalizeHist(src)), R.equalize_hist(grey))


@pytest.mark.parametrize("size", [s for s, _ in CASES])
def test_equalize_hist_equals_the_statement(vp, size):
    from vision.devmat import DeviceMat
    from vision.utils import color
    ctx = vp.default_context()
    w, h = size
    two = np.where(_image(w, h) < 77, 12, 240).astype(np.uint8)
    for img in (_image(w, h), _image(w, h, "narrow"), _image(w, h, "constant"), two, np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)):
        exp = R.equalize_hist(img)
        host = color.equalize_hist(img)
        assert type(host) is np.ndarray and _same(host, exp), (size, "host entry")
        src = _dev(ctx, img)
        out = color.equalize_hist(src)
        assert isinstance(out, DeviceMat) and out.shape == (h, w) and out.binary is False and out._host is None and src._host is None
        assert _same(np.asarray(out), exp), (size, "device entry")


def test_a_mask_in_gives_a_plain_image_out(vp):
    """a 0 / 255 DeviceMat (`binary`) is an image like any other here: the result is not marked as a mask"""
    from vision.utils import color
    ctx = vp.default_context()
    img = _image(64, 64)
    mask = color.range_threshold(_dev(ctx, img), 100, 255)
    assert mask.binary
    m = np.asarray(mask)
    for out, exp in ((color.clahe(mask, 2.0, (8, 8)), R.clahe(m, 2.0, (8, 8))), (color.equalize_hist(mask), R.equalize_hist(m))):
        assert out.binary is False and _same(np.asarray(out), exp)


def test_clahe_bgr_on_a_device_image_is_the_composition_step_by_step(vp):
    from vision import cv2_facade as f
    from vision.devmat import DeviceMat
    from vision.utils import color
    import frames as F
    ctx = vp.default_context()
    bgr = F.s1_buoy(0, 256, 144)
    src = _dev(ctx, bgr)
    out = color.clahe_bgr(src, 2.0, (8, 8))
    assert isinstance(out, DeviceMat) and out.shape == bgr.shape and out._host is None and src._host is None
    lab = f.cvtColor(_dev(ctx, bgr), f.COLOR_BGR2LAB)
    l, a, b = f.split(lab)
    step = f.cvtColor(f.merge((color.clahe(l, 2.0, (8, 8)), a, b)), f.COLOR_LAB2BGR)
    assert _same(np.asarray(out), np.asarray(step))
    # the L plane in between is the statement's
    assert _same(np.asarray(color.clahe(l, 2.0, (8, 8))), R.clahe(np.asarray(l), 2.0, (8, 8)))
    assert _same(np.asarray(color.clahe_bgr(bgr, 2.0, (8, 8))), np.asarray(out))          # a numpy image: the same bytes


def test_facade_on_numpy_equals_the_statement(vp):
    from vision import cv2_facade as f
    img = _image(37, 29)
    for clip, grid in ((40.0, (8, 8)), (2.0, (4, 3)), (0, (1, 1))):
        c = f.createCLAHE(clipLimit=clip, tileGridSize=grid)
        out = c.apply(img)
        assert type(out) is np.ndarray and _same(out, R.clahe(img, clip, grid))
        dst = np.zeros_like(img)
        assert c.apply(img, dst) is dst and _same(dst, out)
        assert _same(c.apply(img[:, :, None]), out)
    c = f.createCLAHE()
    c.setClipLimit(3.0)
    c.setTilesGridSize((2, 5))
    assert _same(c.apply(img), R.clahe(img, 3.0, (2, 5)))
    assert _same(f.equalizeHist(img), R.equalize_hist(img))
    dst = np.zeros_like(img)
    assert f.equalizeHist(img, dst) is dst and _same(dst, R.equalize_hist(img))
    with pytest.raises(f.error):
        f.createCLAHE(2.0, (8, 8)).apply(np.zeros((4, 4), np.uint8))      # the extension is not smaller than the image


def test_host_entries_through_the_c_abi_and_rejected_device_calls(vp):
    from vision.devmat import DeviceMat
    ctx = vp.default_context()
    L = vp.lib()
    img = _image(37, 29)
    out = np.empty_like(img)
    vp.check(L.vp_clahe_u8(ctx.handle, vp.ptr(img), 37, 29, 2.0, 4, 3, vp.ptr(out)), ctx.handle)
    assert _same(out, R.clahe(img, 2.0, (4, 3)))
    vp.check(L.vp_equalize_hist_u8(ctx.handle, vp.ptr(img), 37, 29, vp.ptr(out)), ctx.handle)
    assert _same(out, R.equalize_hist(img))
    h, w = 20, 64
    before = np.arange(4 * h * w, dtype=np.uint32).astype(np.uint8).reshape(4 * h, w)
    buf = DeviceMat(ctx, (4 * h, w))
    vp.check(L.vp_memcpy_h2d(ctx.handle, buf.dev_ptr, before.ctypes.data, before.nbytes), ctx.handle)

    def fetch():
        """the device bytes themselves: the entries below write through raw pointers, behind any host copy a DeviceMat keeps"""
        got = np.empty_like(before)
        ctx.synchronize()
        vp.check(L.vp_memcpy_d2h(ctx.handle, got.ctypes.data, buf.dev_ptr, got.nbytes), ctx.handle)
        return got
    p = buf.dev_ptr
    INV, UNS = vp.ERR_INVALID, vp.ERR_UNSUPPORTED
    assert L.vp_clahe_dev(ctx.handle, p, w, w, h, 2.0, 8, 4, p + h * w - 1) == INV             # overlap
    assert L.vp_clahe_dev(ctx.handle, p, w - 1, w, h, 2.0, 8, 4, p + 2 * h * w) == INV         # stride
    assert L.vp_clahe_dev(ctx.handle, p, w, w, h, float("nan"), 8, 4, p + 2 * h * w) == INV
    assert L.vp_clahe_dev(ctx.handle, p, w, w, h, 2.0, 65, 4, p + 2 * h * w) == UNS
    assert L.vp_clahe_dev(ctx.handle, p, w, w, 3, 2.0, 8, 8, p + 2 * h * w) == UNS             # extension 5 >= 3 rows
    assert L.vp_clahe_dev(ctx.handle, p, w, w, h, 1e300, 8, 4, p + 2 * h * w) == UNS
    assert L.vp_equalize_hist_dev(ctx.handle, p, w, w, h, p + 5) == INV
    assert L.vp_equalize_hist_dev(ctx.handle, None, w, w, h, p) == INV
    assert _same(fetch(), before), "a rejected call wrote to the image"
    vp.check(L.vp_clahe_dev(ctx.handle, p, w, w, h, 2.0, 8, 4, p + h * w), ctx.handle)        # apart: accepted
    got = fetch()
    assert _same(got[h:2 * h], R.clahe(before[:h], 2.0, (8, 4))) and _same(got[:h], before[:h]) and _same(got[2 * h:], before[2 * h:])
    vp.check(L.vp_equalize_hist_dev(ctx.handle, p, w, w, h, p + 2 * h * w), ctx.handle)
    got = fetch()
    assert _same(got[2 * h:3 * h], R.equalize_hist(before[:h])) and _same(got[:h], before[:h]) and _same(got[3 * h:], before[3 * h:])
