"""GPU suite: cv2.adaptiveThreshold with ADAPTIVE_THRESH_GAUSSIAN_C on the MI355X (csrc/vp_adaptive.hip) equals the statement of the tests
(adaptive_gauss_restate.py) bit for bit through the host, device (strided source) and batch entries, the mirror (numpy and DeviceMat)
and the facade; the facade's ADAPTIVE_THRESH_MEAN_C equals the existing mean entry."""
import numpy as np
import pytest

import adaptive_gauss_restate as R
import frames as F

pytestmark = pytest.mark.gpu

BLOCKS = [3, 5, 7, 9, 11, 31, 151, 255, 511]


def _host(vp, img, max_value, ttype, block, c):
    ctx = vp.default_context()
    img = np.ascontiguousarray(img)
    out = np.full(img.shape, 77, np.uint8)
    vp.check(vp.lib().vp_adaptive_threshold_gaussian_u8(ctx.handle, vp.ptr(img), img.shape[1], img.shape[0], float(max_value), int(ttype),
                                                        int(block), float(c), vp.ptr(out)), ctx.handle)
    return out


def _gray(seed, w, h):
    return np.ascontiguousarray(F.s2_bins(seed, w, h)[:, :, 1])


def _uneven(seed, w, h):
    """A frame with a bright top and a dark bottom plus texture: what adaptive thresholding is for."""
    rng = np.random.default_rng(seed)
    ramp = np.linspace(230, 20, h)[:, None]
    return np.clip(ramp + rng.normal(0, 25, (h, w)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("block", BLOCKS)
def test_blocks_on_odd_sizes(vp, block):
    rng = np.random.default_rng(block)
    for h, w in ((37, 53), (64, 301), (5, 6)):
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        mean = R.gaussian_mean(img, block)
        for ttype in (0, 1):
            for c in (0, 2.5, -3.25, 7):
                exp = R.apply_threshold(img, mean, 255, ttype, c)
                assert np.array_equal(_host(vp, img, 255, ttype, block, c), exp), (h, w, ttype, c)


def test_tiny_and_thin_images(vp):
    rng = np.random.default_rng(5)
    for h, w in ((1, 1), (1, 97), (97, 1), (2, 3), (3, 1), (1, 2)):
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        for block in (3, 11, 511):
            for ttype in (0, 1):
                exp = R.adaptive_threshold_gaussian(img, 255, ttype, block, 0)
                assert np.array_equal(_host(vp, img, 255, ttype, block, 0), exp), (h, w, block, ttype)
                exp = R.adaptive_threshold_gaussian(img, 255, ttype, block, -1)
                assert np.array_equal(_host(vp, img, 255, ttype, block, -1), exp), (h, w, block, ttype)


def test_thin_frames_after_the_tap_cache_is_full(vp):
    # a fresh context keeps 8 block sizes; a one-pixel side needs a second size (the single tap) in the same call, whose insertion must
    # not evict the first one's slot
    rng = np.random.default_rng(21)
    img = rng.integers(0, 256, (40, 60), dtype=np.uint8)
    row = rng.integers(0, 256, (1, 97), dtype=np.uint8)
    col = np.ascontiguousarray(row.reshape(97, 1))
    orders = ([11, 3, 5, 7, 9, 31, 151, 255], [3, 5, 7, 9, 31, 151, 255, 11], [511, 11, 3, 5, 7, 9, 31, 151])
    for order in orders:
        for thin in (row, col):
            for probe in (order[0], order[-1], 13):
                ctx = vp.Context(0)
                try:
                    for b in order:
                        out = np.empty_like(img)
                        vp.check(vp.lib().vp_adaptive_threshold_gaussian_u8(ctx.handle, vp.ptr(img), 60, 40, 255.0, 0, b, 0.0, vp.ptr(out)), ctx.handle)
                        assert np.array_equal(out, R.adaptive_threshold_gaussian(img, 255, 0, b, 0)), b
                    for frame in (thin, img, thin):
                        h, w = frame.shape
                        out = np.empty_like(frame)
                        vp.check(vp.lib().vp_adaptive_threshold_gaussian_u8(ctx.handle, vp.ptr(frame), w, h, 255.0, 1, probe, -1.0, vp.ptr(out)),
                                 ctx.handle)
                        assert np.array_equal(out, R.adaptive_threshold_gaussian(frame, 255, 1, probe, -1)), (order, frame.shape, probe)
                finally:
                    ctx.close()
    # the single tap cached in the slot that is replaced next, then a one-column frame with a block size not cached
    ctx = vp.Context(0)
    try:
        for frame, b in ((col, 3), (img, 5), (img, 7), (img, 9), (img, 31), (img, 151), (img, 255), (col, 11), (row, 511), (img, 3)):
            h, w = frame.shape
            out = np.empty_like(frame)
            vp.check(vp.lib().vp_adaptive_threshold_gaussian_u8(ctx.handle, vp.ptr(frame), w, h, 255.0, 0, b, 0.0, vp.ptr(out)), ctx.handle)
            assert np.array_equal(out, R.adaptive_threshold_gaussian(frame, 255, 0, b, 0)), (frame.shape, b)
    finally:
        ctx.close()


def test_max_value_and_bias(vp):
    img = _uneven(1, 160, 120)
    for block in (3, 11, 31):
        mean = R.gaussian_mean(img, block)
        for mv in (255, 200.4, 0, -1):
            for ttype in (0, 1):
                for c in (0, 0.5, -0.5, 4.2, -7.9):
                    exp = R.apply_threshold(img, mean, mv, ttype, c) if mv >= 0 else np.zeros_like(img)
                    assert np.array_equal(_host(vp, img, mv, ttype, block, c), exp), (block, mv, ttype, c)


@pytest.mark.parametrize("block", [11, 31, 151, 511])
def test_1080p(vp, block):
    img = _uneven(2, 1920, 1080)
    mean = R.gaussian_mean(img, block)
    for ttype, c in ((0, 2), (1, -1.5)):
        assert np.array_equal(_host(vp, img, 255, ttype, block, c), R.apply_threshold(img, mean, 255, ttype, c)), (ttype, c)


def test_4k(vp):
    img = _uneven(3, 3840, 2160)
    assert np.array_equal(_host(vp, img, 255, 0, 31, 3), R.adaptive_threshold_gaussian(img, 255, 0, 31, 3))


def test_device_entry_with_strided_source_and_batch(vp):
    import torch
    ctx = vp.default_context()
    h, w, stride = 90, 130, 160
    fstride = h * stride + 512
    frames = [_uneven(10 + i, w, h) for i in range(3)] + [_gray(4, w, h), np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)]
    flat = np.zeros(len(frames) * fstride, np.uint8)
    for i, fr in enumerate(frames):
        flat[i * fstride:i * fstride + h * stride].reshape(h, stride)[:, :w] = fr
    dev = torch.from_numpy(flat).cuda()
    for block, ttype, c in ((3, 0, 0), (31, 1, 2.5), (151, 0, -4), (511, 1, 0)):
        exps = [R.adaptive_threshold_gaussian(fr, 255, ttype, block, c) for fr in frames]
        out = torch.full((len(frames), h, w), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        vp.check(vp.lib().vp_adaptive_threshold_gaussian_batch_dev(ctx.handle, dev.data_ptr(), stride, fstride, len(frames), w, h, 255.0, ttype,
                                                                   block, float(c), out.data_ptr()), ctx.handle)
        vp.check(vp.lib().vp_synchronize(ctx.handle), ctx.handle)
        got = out.cpu().numpy()
        for i in range(len(frames)):
            assert np.array_equal(got[i], exps[i]), (block, i)
        one = torch.full((h, w), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        vp.check(vp.lib().vp_adaptive_threshold_gaussian_dev(ctx.handle, dev.data_ptr() + fstride, stride, w, h, 255.0, ttype, block, float(c),
                                                             one.data_ptr()), ctx.handle)
        vp.check(vp.lib().vp_synchronize(ctx.handle), ctx.handle)
        assert np.array_equal(one.cpu().numpy(), exps[1]), block


def test_mirror_numpy_and_device(vp):
    from vision.devmat import lazy_enabled, set_lazy
    was = lazy_enabled()
    set_lazy(False)                       # numpy in -> numpy out needs the lazy mode off (VP_LAZY=0)
    try:
        _mirror_numpy_and_device(vp)
    finally:
        set_lazy(was)


def _mirror_numpy_and_device(vp):
    from vision.devmat import DeviceMat
    from vision.utils import color
    img = _uneven(4, 320, 240)
    for block, bias in ((11, 2), (31, -3.5), (151, 0)):
        exp = R.adaptive_threshold_gaussian(img, 255, 0, block, bias)
        exp_inv = R.adaptive_threshold_gaussian(img, 255, 1, block, bias)
        got = color.adaptive_threshold_gaussian(img, block, bias)
        assert isinstance(got, np.ndarray) and np.array_equal(got, exp)
        assert np.array_equal(color.adaptive_threshold_gaussian_inv(img, block, bias), exp_inv)
        dm = DeviceMat.from_host(vp.default_context(), img)
        dout = color.adaptive_threshold_gaussian(dm, block, bias)
        assert isinstance(dout, DeviceMat) and dout.binary
        assert dout._host is None, "the result was downloaded although nothing read it"
        assert np.array_equal(np.asarray(dout), exp)
        assert np.array_equal(np.asarray(color.adaptive_threshold_gaussian_inv(dm, block, bias)), exp_inv)
    assert np.array_equal(color.adaptive_threshold_gaussian(img[:, :, None], 5), R.adaptive_threshold_gaussian(img, 255, 0, 5, 0))
    # the mirror's device path from a bgr_to_gray DeviceMat stays on the device
    bgr = F.s2_bins(6, 320, 240)
    gray, _ = color.bgr_to_gray(DeviceMat.from_host(vp.default_context(), bgr))
    out = color.adaptive_threshold_gaussian(gray, 31, 2)
    assert isinstance(out, DeviceMat)
    assert np.array_equal(np.asarray(out), R.adaptive_threshold_gaussian(np.asarray(gray), 255, 0, 31, 2))


def test_lazy_mode_gives_a_device_mat(vp):
    from vision.devmat import DeviceMat, lazy_enabled, set_lazy
    from vision.utils import color
    img = _uneven(8, 96, 64)
    was = lazy_enabled()
    set_lazy(True)
    try:
        out = color.adaptive_threshold_gaussian_inv(img, 9, 1)
    finally:
        set_lazy(was)
    assert isinstance(out, DeviceMat)
    assert np.array_equal(np.asarray(out), R.adaptive_threshold_gaussian(img, 255, 1, 9, 1))


def test_facade(vp):
    from vision import cv2_facade as cv
    from vision.devmat import DeviceMat, lazy_enabled, set_lazy
    was = lazy_enabled()
    set_lazy(False)
    try:
        _facade(vp, cv, DeviceMat)
    finally:
        set_lazy(was)


def _facade(vp, cv, DeviceMat):
    img = _uneven(9, 200, 150)
    for block in (3, 11, 151, 511):
        for mv in (255, 200.4, 0, -1):
            for ttype in (cv.THRESH_BINARY, cv.THRESH_BINARY_INV):
                got = cv.adaptiveThreshold(img, mv, cv.ADAPTIVE_THRESH_GAUSSIAN_C, ttype, block, -2.5)
                assert np.array_equal(np.asarray(got), R.adaptive_threshold_gaussian(img, mv, ttype, block, -2.5)), (block, mv, ttype)
    dst = np.zeros_like(img)
    got = cv.adaptiveThreshold(img, 255, cv.ADAPTIVE_THRESH_GAUSSIAN_C, cv.THRESH_BINARY, 11, 2, dst)
    assert np.array_equal(dst, R.adaptive_threshold_gaussian(img, 255, 0, 11, 2))
    dm = DeviceMat.from_host(vp.default_context(), img)
    got = cv.adaptiveThreshold(dm, 255, cv.ADAPTIVE_THRESH_GAUSSIAN_C, cv.THRESH_BINARY, 31, 0)
    assert isinstance(got, DeviceMat) and np.array_equal(np.asarray(got), R.adaptive_threshold_gaussian(img, 255, 0, 31, 0))
    with pytest.raises(vp.VpError):
        cv.adaptiveThreshold(img, 255, cv.ADAPTIVE_THRESH_GAUSSIAN_C, cv.THRESH_BINARY, 513, 0)


def test_facade_mean_equals_the_mean_entry(vp):
    from vision import cv2_facade as cv
    ctx = vp.default_context()
    img = _uneven(11, 180, 130)
    for block in (3, 11, 151):
        for mv, ttype, c in ((255, 0, 0), (200.4, 1, 2.5), (17, 0, -3.5)):
            exp = np.empty_like(img)
            vp.check(vp.lib().vp_adaptive_threshold_mean_u8(ctx.handle, vp.ptr(img), 180, 130, float(mv), ttype, block, float(c), vp.ptr(exp)),
                     ctx.handle)
            got = cv.adaptiveThreshold(img, mv, cv.ADAPTIVE_THRESH_MEAN_C, ttype, block, c)
            assert np.array_equal(got, exp), (block, mv, ttype, c)


def test_invalid_arguments_are_errors(vp):
    ctx = vp.default_context()
    L = vp.lib()
    img = np.zeros((20, 30), np.uint8)
    out = np.zeros_like(img)

    def call(w=30, h=20, mv=255.0, t=0, b=3, c=0.0):
        return L.vp_adaptive_threshold_gaussian_u8(ctx.handle, vp.ptr(img), w, h, mv, t, b, c, vp.ptr(out))
    assert call() == 0
    for kw in (dict(w=0), dict(h=-1), dict(t=2), dict(b=1), dict(b=4), dict(b=-3), dict(mv=float("nan")), dict(c=float("inf")), dict(c=2e6)):
        assert call(**kw) == -1, kw
    assert call(b=513) == -4
    assert L.vp_adaptive_threshold_gaussian_dev(ctx.handle, None, 30, 30, 20, 255.0, 0, 3, 0.0, vp.ptr(out)) == -1
    assert L.vp_adaptive_threshold_gaussian_batch_dev(ctx.handle, vp.ptr(img), 30, 600, 0, 30, 20, 255.0, 0, 3, 0.0, vp.ptr(out)) == -1
