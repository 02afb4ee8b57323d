"""GPU suite for cv2.medianBlur (vp_median_blur_u8 / vp_median_blur_dev, vision.utils.transform.median_blur, cv2_facade.medianBlur).

Every comparison is byte for byte.  Expectations come from tests/median_restate.py (the definition in numpy, and the summed-area
majority vote for masks), never from the library under test.  The tiles of the three kernels are at most 256 result bytes wide and
32 rows high (the histogram kernel: 64 byte columns, strips of max(32, ksize) rows), so 77 x 300 and 300 x 77 cover more than one
tile and a ragged remainder in either direction for every kernel; no shape had to be enlarged."""
import ctypes as C
import functools

import numpy as np
import pytest

from median_restate import majority_restate, median_restate

pytestmark = pytest.mark.gpu

SMALL = [(1, 1), (1, 7), (7, 1), (2, 3), (5, 4), (37, 29), (77, 300), (300, 77)]      # (h, w)
PLANES = [(64, 128), (65, 192)]                                                      # whole words per row: the bit planes
KS = [1, 3, 5, 7, 9, 15, 31, 63]
CONTENTS = ["uniform", "extremes", "hramp", "vramp", "zeros", "ones", "mask02", "mask10", "mask50", "mask98"]


@functools.lru_cache(maxsize=None)
def _image(kind, h, w, cn):
    rng = np.random.default_rng(h * 1009 + w * 31 + cn * 7 + CONTENTS.index(kind))
    shape = (h, w) if cn == 1 else (h, w, cn)
    if kind == "uniform":
        a = rng.integers(0, 256, shape, dtype=np.uint8)
    elif kind == "extremes":                          # long runs of equal keys through the networks, bin boundaries in the histograms
        a = rng.choice(np.array([0, 1, 254, 255], np.uint8), shape)
    elif kind == "hramp":
        a = np.broadcast_to((np.arange(w) * 255 // max(w - 1, 1)).astype(np.uint8).reshape((1, w) + (1,) * (len(shape) - 2)), shape)
    elif kind == "vramp":
        a = np.broadcast_to((np.arange(h) * 255 // max(h - 1, 1)).astype(np.uint8).reshape((h, 1) + (1,) * (len(shape) - 2)), shape)
    elif kind == "zeros":
        a = np.zeros(shape, np.uint8)
    elif kind == "ones":
        a = np.full(shape, 255, np.uint8)
    else:
        a = np.where(rng.random(shape) < int(kind[4:]) / 100.0, 255, 0).astype(np.uint8)
    a = np.ascontiguousarray(a)
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def _expect(kind, h, w, cn, k):
    out = median_restate(_image(kind, h, w, cn), k)
    out.flags.writeable = False
    return out


def _dev(ctx, arr, binary=False):
    from vision.devmat import DeviceMat
    return DeviceMat.from_host(ctx, arr, binary=binary)


def _both_forms(ctx, img, k):
    """the host entry (numpy in, numpy out) and the device entry (DeviceMat in, DeviceMat out) of one call"""
    from vision.devmat import DeviceMat
    from vision.utils.transform import median_blur
    host = median_blur(img, k)
    assert type(host) is np.ndarray and host.dtype == np.uint8 and host.shape == img.shape
    src = _dev(ctx, img)
    out = median_blur(src, k)
    assert isinstance(out, DeviceMat) and out.shape == img.shape and out._host is None and src._host is None
    return host, np.asarray(out)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("cn", [1, 3, 4])
@pytest.mark.parametrize("hw", SMALL)
def test_random_bytes_equal_the_restatement(vp, hw, cn, k):
    ctx = vp.default_context()
    h, w = hw
    host, dev = _both_forms(ctx, _image("uniform", h, w, cn), k)
    exp = _expect("uniform", h, w, cn, k)
    assert np.array_equal(host, exp), (hw, cn, k, "host entry")
    assert np.array_equal(dev, exp), (hw, cn, k, "device entry")


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("hw", SMALL)
def test_two_channels_at_3_and_5(vp, hw, k):
    ctx = vp.default_context()
    h, w = hw
    host, dev = _both_forms(ctx, _image("uniform", h, w, 2), k)
    exp = _expect("uniform", h, w, 2, k)
    assert np.array_equal(host, exp) and np.array_equal(dev, exp), (hw, k)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind", CONTENTS[1:])
@pytest.mark.parametrize("hw", SMALL)
def test_other_contents_equal_the_restatement(vp, hw, kind, k):
    ctx = vp.default_context()
    h, w = hw
    from vision.utils.transform import median_blur
    out = median_blur(_dev(ctx, _image(kind, h, w, 1)), k)
    assert np.array_equal(np.asarray(out), _expect(kind, h, w, 1, k)), (hw, kind, k)
    if hw == (37, 29) and kind in ("extremes", "hramp", "mask50"):
        out = median_blur(_dev(ctx, _image(kind, h, w, 3)), k)
        assert np.array_equal(np.asarray(out), _expect(kind, h, w, 3, k)), (hw, kind, k, 3)


def test_window_255_where_everything_clamps(vp):
    """9 x 6: every window position but a few is a clamped one, and on a constant image one 16-bit bin holds all 65,025 counts"""
    ctx = vp.default_context()
    for cn in (1, 3):
        for kind in ("uniform", "extremes", "zeros", "ones"):
            img = _image(kind, 9, 6, cn)
            host, dev = _both_forms(ctx, img, 255)
            exp = _expect(kind, 9, 6, cn, 255)
            assert np.array_equal(host, exp) and np.array_equal(dev, exp), (cn, kind)
    img = np.full((9, 6), 7, np.uint8)
    host, dev = _both_forms(ctx, img, 255)
    assert np.array_equal(host, img) and np.array_equal(dev, img)


def test_facade_types_and_dst(vp):
    from vision import cv2_facade
    from vision.devmat import DeviceMat
    ctx = vp.default_context()
    img = _image("uniform", 37, 29, 3)
    exp = _expect("uniform", 37, 29, 3, 5)
    host = cv2_facade.medianBlur(img, 5)
    assert type(host) is np.ndarray and np.array_equal(host, exp)
    out = cv2_facade.medianBlur(_dev(ctx, img), 5)
    assert isinstance(out, DeviceMat) and np.array_equal(np.asarray(out), exp)
    dst = np.zeros_like(img)
    assert cv2_facade.medianBlur(img, 5, dst) is dst and np.array_equal(dst, exp)
    two = _image("uniform", 37, 29, 2)
    assert np.array_equal(cv2_facade.medianBlur(two, 5), _expect("uniform", 37, 29, 2, 5))


def test_strided_source_through_the_c_abi(vp):
    """A column window of a wider device buffer (src_stride > w * cn) gives the bytes of the packed case, for every kernel."""
    from vision.devmat import DeviceMat
    ctx = vp.default_context()
    L = vp.lib()
    rng = np.random.default_rng(5)
    h, x0, w = 45, 31, 67
    for cn, W in ((1, 200), (3, 200), (4, 200), (1, 201), (3, 333)):      # (a stride that is no multiple of 4: every row starts at another phase)
        wide = rng.integers(0, 256, (h, W, cn), dtype=np.uint8)
        win = np.ascontiguousarray(wide[:, x0:x0 + w])
        buf = _dev(ctx, wide)
        for k in (1, 3, 5, 7, 15):
            out = DeviceMat(ctx, (h, w, cn))
            vp.check(L.vp_median_blur_dev(ctx.handle, buf.dev_ptr + x0 * cn, W * cn, w, h, cn, k, 0, None, out.dev_ptr, None, None), ctx.handle)
            exp = median_restate(win, k)
            assert np.array_equal(np.asarray(out), exp), (cn, k)
    W = 200
    wide = np.where(rng.random((h, W)) < 0.4, 255, 0).astype(np.uint8)
    win = np.ascontiguousarray(wide[:, x0:x0 + w])
    buf = _dev(ctx, wide)
    for k in (3, 5, 31, 63):
        out = DeviceMat(ctx, (h, w))
        made = C.c_int(-1)
        vp.check(L.vp_median_blur_dev(ctx.handle, buf.dev_ptr + x0, W, w, h, 1, k, 1, None, out.dev_ptr, None, C.byref(made)), ctx.handle)
        assert made.value == 0
        assert np.array_equal(np.asarray(out), majority_restate(win, k)), k


def test_overlapping_source_and_destination_are_rejected(vp):
    from vision.devmat import DeviceMat
    ctx = vp.default_context()
    L = vp.lib()
    h, w = 20, 64
    buf = DeviceMat(ctx, (2 * h, w))
    before = np.arange(2 * h * w, dtype=np.uint32).astype(np.uint8).reshape(2 * h, w)
    vp.check(L.vp_memcpy_h2d(ctx.handle, buf.dev_ptr, before.ctypes.data, before.nbytes), ctx.handle)
    made = C.c_int(-7)
    for off in (0, 16, (h - 1) * w, h * w - 1):
        rc = L.vp_median_blur_dev(ctx.handle, buf.dev_ptr, w, w, h, 1, 3, 0, None, buf.dev_ptr + off, None, C.byref(made))
        assert rc == vp.ERR_INVALID and made.value == -7, off
    ctx.synchronize()
    after = np.empty_like(before)
    vp.check(L.vp_memcpy_d2h(ctx.handle, after.ctypes.data, buf.dev_ptr, after.nbytes), ctx.handle)
    assert np.array_equal(after, before), "a rejected call wrote to the image"
    rc = L.vp_median_blur_dev(ctx.handle, buf.dev_ptr, w, w, h, 1, 3, 0, None, buf.dev_ptr + h * w, None, None)      # apart: accepted
    assert rc == vp.OK
    ctx.synchronize()


# ---- masks ---------------------------------------------------------------------------------------------------------------------------
def _threshold_source(ctx, h, w, density, seed):
    """a grey device image, the mask range_threshold(150, 255) makes of it, and that mask on the host"""
    from vision.utils.color import range_threshold
    rng = np.random.default_rng(seed)
    gray = np.where(rng.random((h, w)) < density, 200, 10).astype(np.uint8)
    mask = range_threshold(_dev(ctx, gray), 150, 255)
    return mask, np.where(gray >= 150, 255, 0).astype(np.uint8)


@pytest.mark.parametrize("density", [0.02, 0.10, 0.50, 0.98])
@pytest.mark.parametrize("hw", SMALL + PLANES)
def test_masks_are_a_majority_vote_whatever_the_dispatch(vp, hw, density):
    """range_threshold -> median_blur: the result is a mask, equals the majority vote, and the general kernels (VP_OPT_MEDIAN_MASK 0)
    and the forced mask kernel (1: with the bit plane where rows are whole words, from the bytes elsewhere) give the same bytes."""
    from vision.devmat import DeviceMat
    from vision.utils.transform import median_blur
    ctx = vp.default_context()
    h, w = hw
    try:
        for k in (3, 5, 7, 15, 31, 63):
            mask, host_mask = _threshold_source(ctx, h, w, density, 100 * k + h)
            assert mask.binary and (mask._bits is not None) == (w % 64 == 0)
            exp = majority_restate(host_mask, k)
            for opt in (-1, 0, 1):
                ctx.set_option(vp.OPT_MEDIAN_MASK, opt)
                out = median_blur(mask, k)
                assert isinstance(out, DeviceMat) and out.binary, (hw, k, opt)
                assert (out._bits is not None) == (opt != 0 and w % 64 == 0), (hw, k, opt)      # (whole words: the source brought a plane)
                assert np.array_equal(np.asarray(out), exp), (hw, density, k, opt)
            # a mask that came without a plane: the kernel packs its tile from the bytes (and still leaves the result's plane)
            ctx.set_option(vp.OPT_MEDIAN_MASK, 1)
            out = median_blur(_dev(ctx, host_mask, binary=True), k)
            assert (out._bits is not None) == (w % 64 == 0)
            assert np.array_equal(np.asarray(out), exp), (hw, density, k, "from bytes")
    finally:
        ctx.set_option(vp.OPT_MEDIAN_MASK, -1)


def _plane_words(vp, ctx, m):
    h, w = m.shape
    words = np.empty(h * (w // 64), np.uint64)
    vp.check(vp.lib().vp_memcpy_d2h(ctx.handle, words.ctypes.data, m._bits.ptr, words.nbytes), ctx.handle)
    return words.reshape(h, w // 64)


@pytest.mark.parametrize("hw", PLANES)
def test_the_emitted_bit_plane_is_the_results(vp, hw):
    """The labelling and the contour pass read the plane median_blur left: same counts, statistics and contours as on a fresh upload of
    the result's bytes (which has no plane), and the plane's words are the packed bytes."""
    from vision.utils.feature import connected_components, find_contours
    from vision.utils.transform import median_blur
    ctx = vp.default_context()
    h, w = hw
    mask, _ = _threshold_source(ctx, h, w, 0.45, 77)
    out = median_blur(mask, 5)
    assert out._bits is not None
    data = out.host_copy()
    assert out._bits is not None and out._dev_ok
    packed = np.packbits((data != 0).reshape(h, w // 64, 64), axis=2, bitorder="little").view(np.uint64).reshape(h, w // 64)
    assert np.array_equal(_plane_words(vp, ctx, out), packed)
    fresh = _dev(ctx, data, binary=True)
    assert fresh._bits is None
    n1, l1, s1, c1 = connected_components(out)
    n2, l2, s2, c2 = connected_components(fresh)
    assert n1 == n2 and n1 > 1 and np.array_equal(s1, s2) and np.array_equal(c1, c2, equal_nan=True) and np.array_equal(np.asarray(l1), np.asarray(l2))
    k1 = find_contours(out, vp.RETR_EXTERNAL)
    k2 = find_contours(fresh, vp.RETR_EXTERNAL)
    assert len(k1) == len(k2) and len(k1) > 0 and all(np.array_equal(a, b) for a, b in zip(k1, k2))


def test_end_to_end_despeckle_then_label(vp):
    """192 x 256 grey: one 40 x 40 square at 200 under 10 % salt at 255 -> range_threshold(150, 255) -> median_blur(3) ->
    connected_components, on device images and on numpy inputs with the restatement standing in for the filter."""
    from vision.utils.color import range_threshold
    from vision.utils.feature import connected_components
    from vision.utils.transform import median_blur
    ctx = vp.default_context()
    rng = np.random.default_rng(9)
    img = np.full((192, 256), 20, np.uint8)
    img[70:110, 100:140] = 200
    img[rng.random(img.shape) < 0.10] = 255
    dm = median_blur(range_threshold(_dev(ctx, img), 150, 255), 3)
    assert dm.binary and dm._bits is not None
    n1, l1, s1, c1 = connected_components(dm)
    host_mask = np.asarray(range_threshold(img, 150, 255))
    assert np.array_equal(host_mask, np.where(img >= 150, 255, 0).astype(np.uint8))
    filtered = median_restate(host_mask, 3)
    n2, l2, s2, c2 = connected_components(filtered)
    assert np.array_equal(np.asarray(dm), filtered)
    assert n1 == n2 and np.array_equal(s1, s2) and np.array_equal(c1, c2, equal_nan=True) and np.array_equal(np.asarray(l1), np.asarray(l2))
    assert s1[1:, 4].max() >= 1500, "the square survived the filter"


def test_full_size_network_and_mask_kernels(vp):
    from vision.utils.transform import median_blur
    ctx = vp.default_context()
    rng = np.random.default_rng(10)
    img = rng.integers(0, 256, (1080, 1920), dtype=np.uint8)
    out = median_blur(_dev(ctx, img), 3)
    assert np.array_equal(np.asarray(out), median_restate(img, 3))
    mask, host_mask = _threshold_source(ctx, 1080, 1920, 0.10, 11)
    out = median_blur(mask, 3)
    assert out.binary and out._bits is not None
    assert np.array_equal(np.asarray(out), median_restate(host_mask, 3))


def test_environment_switch_is_read_when_a_context_is_made(vp):
    """VP_OPT_MEDIAN_MASK in the environment: 0 keeps a new context off the mask kernel (no plane comes back), 1 and nothing put it on."""
    import os
    from vision.devmat import DeviceMat, _DevBuf
    L = vp.lib()
    h, w = 64, 128
    rng = np.random.default_rng(21)
    mask = np.where(rng.random((h, w)) < 0.3, 255, 0).astype(np.uint8)
    exp = majority_restate(mask, 5)
    old = os.environ.get("VP_OPT_MEDIAN_MASK")
    try:
        for value, want in (("0", 0), ("1", 1), (None, 1)):
            if value is None:
                os.environ.pop("VP_OPT_MEDIAN_MASK", None)
            else:
                os.environ["VP_OPT_MEDIAN_MASK"] = value
            ctx = vp.Context(0)
            try:
                src, out, plane = DeviceMat.from_host(ctx, mask), DeviceMat(ctx, (h, w)), _DevBuf(ctx, h * (w // 64) * 8)
                made = C.c_int(-1)
                vp.check(L.vp_median_blur_dev(ctx.handle, src.dev_ptr, w, w, h, 1, 5, 1, None, out.dev_ptr, plane.ptr, C.byref(made)), ctx.handle)
                assert made.value == want, value
                assert np.array_equal(np.asarray(out), exp), value
                del src, out, plane
            finally:
                ctx.close()
    finally:
        if old is None:
            os.environ.pop("VP_OPT_MEDIAN_MASK", None)
        else:
            os.environ["VP_OPT_MEDIAN_MASK"] = old
