"""GPU suite for the colour-histogram family (vp_calc_hist_*, vp_back_project_*, vp_mean_shift_dev; vision.utils.color /
vision.utils.feature; vision.cv2_facade calcHist, calcBackProject, meanShift, CamShift).

Every comparison is exact: tobytes() / integer equality against tests/hist_restate.py, never against the library under test.  Each
histogram and back-projection is taken three ways - the host entry, the device entry on padded strides with 255s in the padding that
would show if they were read, the facade on a device image - and the three must equal the statement.  The shapes are the smallest at
which a kernel can go wrong: a pixel, a row, widths round the four pixels a lane takes, histogram sizes one below, at and one above the
two LDS limits read from csrc/vp_hist_plan.h, and the two 4096 x 4096 images where a count reaches 2^24 and a moment needs 64 bits."""
import itertools
import os
import re

import numpy as np
import pytest

import hist_restate as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PLAN = open(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc", "vp_hist_plan.h")).read()
_num = lambda n: int(re.search(r"#define " + n + r" (\d+)", _PLAN).group(1))
HIST_LDS_BINS, BP_LDS_BYTES, PX = _num("HS_HIST_LDS_BINS"), _num("HS_BP_LDS_BYTES"), _num("HS_PX")
assert "P->in_lds = P->total <= HS_HIST_LDS_BINS;" in _PLAN and "P->in_lds = P->total <= HS_BP_LDS_BYTES;" in _PLAN
CRIT = (3, 10, 1.0)                                   # TERM_CRITERIA_COUNT | TERM_CRITERIA_EPS


def _three_sizes(n):
    """three sizes of 1..256 whose product is n, the largest first"""
    for a in range(1, 257):
        if n % a == 0:
            for b in range(a, 257):
                if (n // a) % b == 0 and (n // a) // b <= 256:
                    return ((n // a) // b, b, a)
    raise AssertionError(n)


def _random(h, w, cn, seed=0, top=256):
    a = np.random.default_rng(h * 8191 + w * 131 + cn * 7 + seed).integers(0, top, (h, w, cn), dtype=np.uint8)
    return a if cn > 1 else a[:, :, 0]


def _dev(ctx, arr):
    from vision.devmat import DeviceMat
    return DeviceMat.from_host(ctx, arr)


def _padded(ctx, arr, pad, fill):
    """the array in rows of pad more bytes on the device, and its stride in bytes"""
    rows = arr.reshape(arr.shape[0], -1)
    wide = np.full((rows.shape[0], rows.shape[1] + pad), fill, np.uint8)
    wide[:, :rows.shape[1]] = rows
    return _dev(ctx, wide), wide.shape[1]


def _desc(channels, sizes, ranges):
    keep = (np.array(channels, np.int32), np.array(sizes, np.int32), np.array(ranges, np.float64).reshape(-1))
    return (len(channels), keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data), keep


def _cn(img):
    return 1 if img.ndim == 2 else img.shape[2]


def _hist_device_entry(vp, img, channels, sizes, ranges, mask=None, bits=None, pad=5):
    """vp_calc_hist_dev on padded rows, the counts left in device memory and copied to the host in the same call"""
    ctx = vp.default_context()
    h, w = img.shape[:2]
    src, stride = _padded(ctx, img, pad, 255)
    mp, ms = (None, 0) if mask is None else _padded(ctx, mask, 3, 255)
    bp = None if bits is None else _dev(ctx, bits)
    total = int(np.prod(sizes))
    left = _dev(ctx, np.full(total + 2, 0xdeadbeef, np.uint32))
    back = np.empty(tuple(sizes), np.uint32)
    args, keep = _desc(channels, sizes, ranges)
    have = mask is not None or bits is not None
    rc = vp.lib().vp_calc_hist_dev(ctx.handle, src.dev_ptr, stride, w, h, _cn(img), *args, None if mp is None else mp.dev_ptr, ms, w if have else 0,
                                   h if have else 0, None if bp is None else bp.dev_ptr, left.dev_ptr, back.ctypes.data)
    vp.check(rc, ctx.handle)
    got = left.host_copy()
    assert (got[total:] == 0xdeadbeef).all(), "counters past the histogram were written"
    assert got[:total].tobytes() == back.tobytes(), "the device and the host copy of the counts differ"
    return back


def _hist_three_ways(vp, img, channels, sizes, ranges, mask=None):
    from vision import cv2_facade as f
    from vision.utils import color
    ctx = vp.default_context()
    exp = R.calc_hist_counts(img, channels, sizes, ranges, mask)
    tag = (img.shape, channels, sizes, ranges)
    got = color.color_histogram(img, channels, sizes, ranges, mask)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == tuple(sizes) and got.tobytes() == exp.astype(np.float32).tobytes(), tag + ("host",)
    assert _hist_device_entry(vp, img, channels, sizes, ranges, mask).tobytes() == exp.tobytes(), tag + ("device, padded strides",)
    src = _dev(ctx, img)
    dgot = f.calcHist([src], list(channels), None if mask is None else _dev(ctx, mask), list(sizes), list(ranges))
    assert isinstance(dgot, np.ndarray) and dgot.dtype == np.float32 and dgot.tobytes() == exp.astype(np.float32).tobytes(), tag + ("facade, device image",)
    assert src._host is None, "a host copy of the source was made"
    return exp


def _bp_device_entry(vp, img, channels, hist, ranges, scale, pad=5, dpad=3):
    ctx = vp.default_context()
    h, w = img.shape[:2]
    src, stride = _padded(ctx, img, pad, 255)
    dst = _dev(ctx, np.full((h, w + dpad), 90, np.uint8))
    dh = _dev(ctx, np.ascontiguousarray(hist, np.float32))
    args, keep = _desc(channels, hist.shape, ranges)
    vp.check(vp.lib().vp_back_project_dev(ctx.handle, src.dev_ptr, stride, w, h, _cn(img), *args, dh.dev_ptr, float(scale), dst.dev_ptr, w + dpad), ctx.handle)
    got = dst.host_copy()
    assert (got[:, w:] == 90).all(), "the result's padding was written"
    return np.ascontiguousarray(got[:, :w])


def _bp_three_ways(vp, img, channels, hist, ranges, scale):
    from vision import cv2_facade as f
    from vision.devmat import DeviceMat
    from vision.utils import color
    ctx = vp.default_context()
    exp = R.back_project(img, channels, hist, ranges, scale)
    tag = (img.shape, channels, hist.shape, ranges, scale)
    got = color.back_project(img, channels, hist, ranges, scale)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == exp.shape and got.tobytes() == exp.tobytes(), tag + ("host",)
    assert _bp_device_entry(vp, img, channels, hist, ranges, scale).tobytes() == exp.tobytes(), tag + ("device, padded strides",)
    src = _dev(ctx, img)
    dgot = f.calcBackProject([src], list(channels), hist, list(ranges), scale)
    assert isinstance(dgot, DeviceMat) and dgot.dtype == np.uint8 and dgot.shape == exp.shape
    assert dgot.host(writable=False).tobytes() == exp.tobytes(), tag + ("facade, device image",)
    assert src._host is None, "a host copy of the source was made"
    model = color.HistModel(hist, channels, ranges, scale)
    applied = model.apply(src)
    assert isinstance(applied, DeviceMat) and applied.host(writable=False).tobytes() == exp.tobytes(), tag + ("HistModel.apply",)
    return exp


# ---- histogram -------------------------------------------------------------------------------------------------------------------

def test_small_images_and_widths_round_a_lanes_pixels(vp):
    for h, w in ((1, 1), (1, 257), (3, 5), (2, PX - 1), (2, PX), (2, PX + 1), (5, 8 * PX - 1), (5, 8 * PX + 1)):
        for cn in (1, 3):
            img = _random(h, w, cn)
            _hist_three_ways(vp, img, (cn - 1,), (16,), (0, 256))
            if cn == 3:
                _hist_three_ways(vp, img, (0, 2), (5, 7), (0, 256, 10.5, 200.25))


@pytest.mark.parametrize("dims", (1, 2, 3))
def test_every_channel_choice(vp, dims):
    sizes, ranges = (6, 5, 4)[:dims], (0, 256, 10.5, 200.25, 0, 180)[:2 * dims]
    for cn in (1, 2, 3, 4):
        img = _random(5, 7, cn, seed=dims)
        for channels in itertools.product(range(cn), repeat=dims):
            exp = R.calc_hist_counts(img, channels, sizes, ranges)
            assert _hist_device_entry(vp, img, channels, sizes, ranges).tobytes() == exp.tobytes(), (cn, channels)
        _hist_three_ways(vp, img, tuple(range(cn))[-dims:] if cn >= dims else (0,) * dims, sizes, ranges)


def test_total_bins_round_the_lds_limit(vp):
    img = _random(33, 47, 3)
    for total in (HIST_LDS_BINS - 1, HIST_LDS_BINS, HIST_LDS_BINS + 1):
        sizes = _three_sizes(total)
        exp = _hist_three_ways(vp, img, (0, 1, 2), sizes, (0, 256, 0, 256, 0, 256))
        assert exp.sum() == 33 * 47
    for sizes, channels in (((180, 256), (0, 1)), ((32, 32, 32), (0, 1, 2)), ((256, 256), (2, 0))):          # the typical ones, either side of the limit
        _hist_three_ways(vp, img, channels, sizes, (0, 256) * len(sizes))


def test_a_uniform_image_and_one_without_a_pixel_in_range(vp):
    for sizes in ((180, 256), (32, 32)):                                     # device counters, LDS counters
        img = np.full((37, 130, 3), (90, 200, 7), np.uint8)
        exp = _hist_three_ways(vp, img, (0, 1), sizes, (0, 180, 0, 256))
        assert np.count_nonzero(exp) == 1 and exp.max() == 37 * 130
        exp = _hist_three_ways(vp, img, (0, 1), sizes, (0, 90, 0, 256))      # 90 is the exclusive end: nothing is counted
        assert exp.sum() == 0
        img[5, 7] = (91, 0, 0)                                               # one lane of one wave breaks its run
        exp = _hist_three_ways(vp, img, (0, 1), sizes, (0, 180, 0, 256))
        assert np.count_nonzero(exp) == 2 and exp.sum() == 37 * 130


def test_hue_like_and_fractional_ranges(vp):
    hsv = _random(21, 35, 3, seed=4)
    hsv[:, :, 0] %= 200                                                      # hue-like, with values at and past the exclusive 180
    hsv[0, 0, 0], hsv[0, 1, 0] = 179, 180
    _hist_three_ways(vp, hsv, (0,), (180,), (0, 180))
    _hist_three_ways(vp, hsv, (0, 1), (180, 256), (0, 180, 0, 256))
    _hist_three_ways(vp, hsv, (1,), (7,), (10.5, 200.25))
    _hist_three_ways(vp, hsv, (2, 1), (7, 3), (10.5, 200.25, -20, 300))


@pytest.mark.parametrize("w", (64, 128, 65))
def test_a_byte_mask_and_its_bit_plane(vp, w):
    from vision.utils import color
    ctx = vp.default_context()
    h = 9
    img = _random(h, w, 3, seed=w)
    grey = _random(h, w, 1, seed=w + 1)
    mask = np.where(grey > 100, 255, 0).astype(np.uint8)
    mask[:, -1] = 255
    exp = _hist_three_ways(vp, img, (0, 2), (8, 9), (0, 256, 0, 256), mask)
    assert 0 < exp.sum() == np.count_nonzero(mask) < h * w
    odd = mask.copy()
    odd[odd != 0] = 3                                                        # any non-zero byte counts
    assert _hist_device_entry(vp, img, (0, 2), (8, 9), (0, 256, 0, 256), odd).tobytes() == exp.tobytes()
    # the plane alone, and beside the bytes (then the plane is read): rows of ceil(w / 64) words, the bits past w set
    words = (w + 63) // 64
    wide = np.ones((h, words * 64), bool)
    wide[:, :w] = mask != 0
    bits = np.packbits(wide, axis=1, bitorder="little").view(np.uint64).reshape(h, words)
    assert _hist_device_entry(vp, img, (0, 2), (8, 9), (0, 256, 0, 256), None, bits).tobytes() == exp.tobytes()
    assert _hist_device_entry(vp, img, (0, 2), (8, 9), (0, 256, 0, 256), np.zeros_like(mask), bits).tobytes() == exp.tobytes()
    # a mask made on the device carries its plane when w % 64 == 0; with or without it the result is the same
    dmask = color.range_threshold(_dev(ctx, grey), 101, 255)
    assert (dmask.bit_plane(ctx) is not None) == (w % 64 == 0)
    plain = R.calc_hist(img, (0, 2), (8, 9), (0, 256, 0, 256), np.where(grey > 100, 255, 0))
    assert color.color_histogram(_dev(ctx, img), (0, 2), (8, 9), (0, 256, 0, 256), dmask).tobytes() == plain.tobytes()
    assert color.color_histogram(_dev(ctx, img), (0, 2), (8, 9), (0, 256, 0, 256), _dev(ctx, dmask.host_copy())).tobytes() == plain.tobytes()


def test_a_count_of_2_to_the_24_in_one_bin(vp):
    from vision.utils import color
    ctx = vp.default_context()
    img = np.full((4096, 4096), 77, np.uint8)
    got = color.color_histogram(_dev(ctx, img), (0,), (256,), (0, 256))
    assert got[77] == np.float32(2 ** 24) and np.count_nonzero(got) == 1
    assert got.tobytes() == R.calc_hist(img, (0,), (256,), (0, 256)).tobytes()
    assert _hist_device_entry(vp, img, (0,), (256,), (0, 256), pad=0)[77] == 2 ** 24


# ---- back-projection -------------------------------------------------------------------------------------------------------------

def test_table_sizes_round_the_lds_limit(vp):
    img = _random(19, 41, 3)
    for total in (BP_LDS_BYTES - 1, BP_LDS_BYTES, BP_LDS_BYTES + 1):
        sizes = _three_sizes(total)
        hist = np.random.default_rng(total).integers(0, 300, sizes).astype(np.float32)
        _bp_three_ways(vp, img, (0, 1, 2), hist, (0, 256, 0, 256, 0, 256), 1.0)
    for sizes, channels in (((180, 256), (0, 1)), ((32, 32, 32), (2, 1, 0)), ((64, 64, 64), (0, 1, 2))):
        hist = np.random.default_rng(sizes[0]).integers(0, 300, sizes).astype(np.float32)
        _bp_three_ways(vp, img, channels, hist, (0, 256) * len(sizes), 1.0)


def test_fractions_ties_saturation_and_pixels_out_of_range(vp):
    from vision.utils import color
    img = _random(13, 2 * PX + 1, 3, seed=2)
    counts = (np.arange(30, dtype=np.float32).reshape(6, 5) * 3) % 8        # counts of 0..7: 255 / 7 per count leaves fractions
    stretched = R.normalize_hist(counts, 255)
    assert color.normalize_hist(counts, 255).tobytes() == stretched.tobytes() and (stretched != np.floor(stretched)).any()
    _bp_three_ways(vp, img, (0, 1), stretched, (0, 256, 0, 256), 1.0)
    ties = np.arange(30, dtype=np.float32).reshape(6, 5)                     # times 0.5: every second one a tie; times 20: above 255
    for scale in (0.5, 1.5, 20.0, -1.0, 0.0):
        _bp_three_ways(vp, img, (0, 1), ties, (0, 256, 0, 256), scale)
    exp = _bp_three_ways(vp, img, (0, 1), ties + 1, (0, 128, 64, 256), 1.0)   # pixels without a bin give 0, every bin at least 1
    assert ((exp == 0) == ((img[:, :, 0] >= 128) | (img[:, :, 1] < 64))).all() and (exp == 0).any() and (exp != 0).any()
    for h, w in ((1, 1), (1, 257), (3, PX - 1), (3, PX + 1)):
        for cn in (1, 2, 4):
            small = _random(h, w, cn, seed=9)
            _bp_three_ways(vp, small, (cn - 1,), np.arange(10, 26, dtype=np.float32), (0, 200), 3.0)


def test_a_model_from_a_patch_in_hbm(vp):
    from vision.devmat import DeviceMat
    from vision.utils import color, feature
    ctx = vp.default_context()
    img = _random(30, 41, 3, seed=5)
    src = _dev(ctx, img)
    patch = img[4:15, 13:22]
    for mask in (None, (np.arange(99).reshape(11, 9) % 3 != 0).astype(np.uint8)):
        model = color.HistModel.from_patch(feature.DeviceCrop(src, 13, 4, 9, 11), (0, 1), (12, 8), (0, 256, 0, 256), mask)
        hist = R.normalize_hist(R.calc_hist(patch, (0, 1), (12, 8), (0, 256, 0, 256), mask), 255)
        assert model.hist.tobytes() == hist.tobytes()
        exp = R.back_project(img, (0, 1), hist, (0, 256, 0, 256), 1.0)
        got = model.apply(src)
        assert isinstance(got, DeviceMat) and got.host(writable=False).tobytes() == exp.tobytes()
        assert color.back_project(src, (0, 1), hist, (0, 256, 0, 256)).host(writable=False).tobytes() == exp.tobytes()
        assert model.apply(img).tobytes() == exp.tobytes()
        assert color.HistModel.from_patch(patch, (0, 1), (12, 8), (0, 256, 0, 256), mask).hist.tobytes() == hist.tobytes()
    assert src._host is None, "the frame visited the host"


# ---- mean shift ------------------------------------------------------------------------------------------------------------------

def _blobs(h=48, w=64):
    p = np.zeros((h, w), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    p[(yy - 30) ** 2 + (xx - 40) ** 2 < 60] = 200
    p[(yy - 8) ** 2 + (xx - 9) ** 2 < 20] = 90
    return p + (_random(h, w, 1, seed=1) >> 6)


def _shift_both(vp, prob, window, max_iter=10, eps=1.0):
    from vision import cv2_facade as f
    from vision.utils import feature
    ctx = vp.default_context()
    exp = R.mean_shift(prob, window, max_iter, eps)
    assert feature.mean_shift(prob, window, max_iter, eps) == exp, (window, max_iter, eps, "host image")
    src = _dev(ctx, prob)
    assert f.meanShift(src, window, (3, max_iter, eps)) == exp, (window, max_iter, eps, "facade, device image")
    assert src._host is None
    # the device entry on a padded stride, the result left in device memory
    wide, stride = _padded(ctx, prob, 7, 255)
    out = _dev(ctx, np.full(7, -1, np.int32))
    win = np.array(window, np.int32)
    vp.check(vp.lib().vp_mean_shift_dev(ctx.handle, wide.dev_ptr, stride, prob.shape[1], prob.shape[0], win.ctypes.data, 1, max_iter, eps, out.dev_ptr, None), ctx.handle)
    vp.check(vp.lib().vp_synchronize(ctx.handle), ctx.handle)
    got = out.host_copy()
    assert (int(got[4]), tuple(int(v) for v in got[:4])) == exp and (got[5:] == -1).all(), (window, "device entry, padded stride")
    return exp


def test_windows_of_one_pixel_one_row_and_partly_outside(vp):
    prob = _blobs()
    for window in ((40, 30, 1, 1), (0, 0, 1, 1), (30, 30, 20, 1), (36, 20, 1, 20), (-5, -7, 20, 22), (50, 35, 40, 40), (33, 25, 13, 11), (1, 2, 17, 9)):
        _shift_both(vp, prob, window)
    for window in ((64, 0, 5, 5), (-5, 0, 5, 5), (0, 48, 5, 5), (3, 3, 0, 5)):
        from vision import cv2_facade as f
        with pytest.raises(f.error):
            f.meanShift(prob, window, CRIT)


def test_first_iteration_max_iter_eps_and_no_mass(vp):
    prob = _blobs()
    assert _shift_both(vp, prob, (33, 23, 14, 14))[0] == 0                   # centred on the blob: converges in the first iteration
    far = _shift_both(vp, prob, (10, 5, 30, 30), 100, 1.0)
    assert far[0] >= 2
    for max_iter in (1, 2, far[0], 0, -4):
        got = _shift_both(vp, prob, (10, 5, 30, 30), max_iter, 0.0)          # eps2 = 0: only the count stops it
        assert got[0] == max(max_iter, 1)
    for eps in (0.4, 1.5, 2.5, 3.0, 50.0, -2.0):
        _shift_both(vp, prob, (10, 5, 30, 30), 20, eps)
    zero = np.zeros((48, 64), np.uint8)
    assert _shift_both(vp, zero, (5, 6, 20, 10)) == (0, (5, 6, 20, 10))
    assert _shift_both(vp, prob, (50, 0, 10, 5)) == R.mean_shift(prob, (50, 0, 10, 5), 10, 1.0)


@pytest.mark.parametrize("n", (1, 2, 65))
def test_a_batch_equals_its_single_windows(vp, n):
    from vision.utils import feature
    ctx = vp.default_context()
    prob = _blobs()
    rng = np.random.default_rng(n)
    windows = [(int(rng.integers(-5, 60)), int(rng.integers(-5, 44)), int(rng.integers(1, 40)), int(rng.integers(1, 40))) for _ in range(n)]
    windows = [wd for wd in windows if R.intersect(wd, 64, 48) != (0, 0, 0, 0)] or [(0, 0, 5, 5)]
    windows = (windows * n)[:n]
    src = _dev(ctx, prob)
    got = feature.mean_shift_many(src, windows, 15, 1.0)
    assert len(got) == n and got == [R.mean_shift(prob, wd, 15, 1.0) for wd in windows]
    assert got == [feature.mean_shift(src, wd, 15, 1.0) for wd in windows]


def test_full_windows_of_255s_need_64_bit_sums(vp):
    from vision.utils import feature
    ctx = vp.default_context()
    prob = np.full((4096, 4096), 255, np.uint8)
    src = _dev(ctx, prob)
    m00, m10, m01 = R.window_sums_fast(prob, (0, 0, 4096, 4096))
    assert m10 == m01 == 255 * 4096 * (4095 * 4096 // 2) > 2 ** 42
    assert feature.mean_shift(src, (0, 0, 4096, 4096), 10, 1.0) == R.mean_shift(prob, (0, 0, 4096, 4096), 10, 1.0) == (0, (0, 0, 4096, 4096))
    # one darker pixel moves nothing on a window of this size, yet every sum must be exact for the step to round as the statement's
    corner = (2048, 2048, 2048, 2048)
    prob[:2049, :] = 0
    prob[:, :2049] = 0
    prob[4000:, 4000:] = 1
    src = _dev(ctx, prob)
    exp = R.mean_shift(prob, corner, 3, 0.0)
    assert feature.mean_shift(src, corner, 3, 0.0) == exp and exp[0] == 3
    exp = R.mean_shift(prob, (100, 200, 3000, 3500), 4, 1.0)
    assert feature.mean_shift(src, (100, 200, 3000, 3500), 4, 1.0) == exp and exp[1][:2] != (100, 200)
    assert src._host is None


def test_a_device_chain_follows_a_coloured_square(vp, monkeypatch):
    from vision.devmat import DeviceMat
    from vision.utils import color, feature

    def frame(x, y):
        bgr = np.full((48, 64, 3), (40, 60, 50), np.uint8) + (_random(48, 64, 3, seed=3) >> 5)
        bgr[y:y + 10, x:x + 10] = (20, 40, 230)
        return bgr

    ctx = vp.default_context()
    first, second = frame(20, 15), frame(25, 18)
    d_first, d_second = _dev(ctx, first), _dev(ctx, second)
    hsv_host = color.bgr_to_hsv(first)[0]
    crop = hsv_host[15:25, 20:30]

    def no_host(self, *a, **k):
        raise AssertionError("an image visited the host")
    monkeypatch.setattr(DeviceMat, "host", no_host)
    monkeypatch.setattr(DeviceMat, "host_copy", no_host)
    hsv1 = color.bgr_to_hsv(d_first)[0]
    model = color.HistModel.from_patch(feature.DeviceCrop(hsv1, 20, 15, 10, 10), (0, 1), (30, 32), (0, 180, 0, 256))
    window = (20, 15, 10, 10)
    for d_frame in (d_first, d_second):
        prob = model.apply(color.bgr_to_hsv(d_frame)[0])
        assert isinstance(prob, DeviceMat)
        _, window = feature.mean_shift(prob, window, 10, 1.0)
    monkeypatch.undo()
    # the square went from (20, 15) to (25, 18); a step of half a pixel rounds to none, so the window may rest up to two pixels short
    assert 22 <= window[0] <= 25 and 16 <= window[1] <= 18 and window[2:] == (10, 10)
    # and the whole chain equals the statement's, from the library's own HSV
    hist = R.normalize_hist(R.calc_hist(crop, (0, 1), (30, 32), (0, 180, 0, 256)), 255)
    assert model.hist.tobytes() == hist.tobytes()
    w = (20, 15, 10, 10)
    for bgr in (first, second):
        _, w = R.mean_shift(R.back_project(color.bgr_to_hsv(bgr)[0], (0, 1), hist, (0, 180, 0, 256), 1.0), w, 10, 1.0)
    assert w == window


# ---- CamShift --------------------------------------------------------------------------------------------------------------------

def test_camshift_on_a_rotated_blob_and_without_mass(vp):
    from vision import cv2_facade as f
    from vision.utils import feature
    ctx = vp.default_context()
    yy, xx = np.mgrid[0:64, 0:64]
    u, v = (xx - 30) * 0.8 + (yy - 36) * 0.6, -(xx - 30) * 0.6 + (yy - 36) * 0.8
    blob = np.where((u / 18.0) ** 2 + (v / 6.0) ** 2 < 1, 220, 0).astype(np.uint8) + (_random(64, 64, 1, seed=8) >> 6)
    for prob, window in ((blob, (20, 25, 20, 20)), (blob, (0, 0, 64, 64)), (blob, (40, 40, 30, 30)), (np.zeros((64, 64), np.uint8), (10, 12, 20, 9))):
        exp = R.cam_shift(prob, window, 10, 1.0)
        got = feature.cam_shift(_dev(ctx, prob), window, 10, 1.0)
        assert got[1] == exp[1], "the window"
        assert got[0] == exp[0], "the box, evaluated on the same host"
        assert f.CamShift(prob, window, (3, 10, 1.0)) == exp
    box, window = R.cam_shift(blob, (20, 25, 20, 20), 10, 1.0)
    assert box[1][1] > 2 * box[1][0] > 0 and 100 < box[2] < 150 and abs(box[0][0] - 30) < 3 and abs(box[0][1] - 36) < 3      # long axis near 127 degrees
    assert R.cam_shift(np.zeros((64, 64), np.uint8), (10, 12, 20, 9), 10, 1.0) == (((0.0, 0.0), (0.0, 0.0), 0.0), (0, 2, 40, 29))
