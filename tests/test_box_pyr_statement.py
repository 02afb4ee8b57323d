"""CPU suite for tests/box_pyr_restate.py, the statement of cv2.boxFilter / blur, pyrDown, pyrUp and integral: it is checked against
independent evaluations (np.pad plus shifted adds, np.cumsum, scipy.ndimage.correlate) and against known answers."""
import numpy as np
import pytest

import box_pyr_restate as R

PAD_MODE = {R.BORDER_REFLECT_101: "reflect", R.BORDER_REPLICATE: "edge", R.BORDER_REFLECT: "symmetric", R.BORDER_CONSTANT: "constant"}


def _pad_axis(a, axis, before, after, mode):
    """np.pad along one axis; a pad longer than the image repeats the reflection, as cv::borderInterpolate's loop does"""
    pw = [(0, 0)] * a.ndim
    pw[axis] = (before, after)
    return np.pad(a, pw, mode=mode)


def _box_by_padding(img, kw, kh, border):
    h, w = img.shape[:2]
    ax, ay = kw // 2, kh // 2
    p = _pad_axis(img.astype(np.int64), 0, ay, kh - 1 - ay, PAD_MODE[border])
    p = _pad_axis(p, 1, ax, kw - 1 - ax, PAD_MODE[border])
    return sum(p[i:i + h, j:j + w] for i in range(kh) for j in range(kw))


@pytest.mark.parametrize("border", R.BOX_BORDERS)
def test_box_sums_equal_padding_plus_shifted_adds(border):
    rng = np.random.default_rng(3)
    for shape, kw, kh in (((3, 5), 9, 9), ((3, 5), 3, 3), ((7, 6), 4, 3), ((7, 6), 2, 2), ((9, 11, 3), 5, 1), ((9, 11, 3), 1, 7), ((1, 1), 3, 3), ((2, 9, 4), 6, 5)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        want = _box_by_padding(img, kw, kh, border)
        got = R.box_filter_restate(img, R.CV_32S, kw, kh, False, border)
        assert got.dtype == np.int32 and np.array_equal(got, want), (shape, kw, kh, border)
        assert np.array_equal(R.box_filter_restate(img, R.CV_64F, kw, kh, False, border), want.astype(np.float64))
        assert np.array_equal(R.box_filter_restate(img, R.CV_32F, kw, kh, False, border), want.astype(np.float32))
        assert np.array_equal(R.box_filter_restate(img, -1, kw, kh, False, border), np.minimum(want, 255).astype(np.uint8))
        assert np.array_equal(R.box_filter_restate(img, R.CV_16S, kw, kh, False, border), np.minimum(want, 32767).astype(np.int16))
        if R.area_is_exact(kw * kh):
            area = kw * kh
            q, rem = np.divmod(2 * want + area, 2 * area)                    # half to even, in integers
            q = q - ((rem == 0) & (q % 2 == 1))
            assert np.array_equal(R.box_filter_restate(img, -1, kw, kh, True, border), q.astype(np.uint8)), (shape, kw, kh, border)


def test_box_refusals_and_the_copy():
    img = np.arange(30, dtype=np.uint8).reshape(5, 6)
    assert np.array_equal(R.box_filter_restate(img, -1, 1, 1, True), img)
    assert np.array_equal(R.box_filter_restate(img, R.CV_16S, 1, 1, False), img.astype(np.int16))
    with pytest.raises(ValueError):
        R.box_filter_restate(img, -1, 3, 3, True, R.BORDER_WRAP)
    with pytest.raises(ValueError):
        R.box_filter_restate(img, R.CV_16S, 3, 3, True)
    with pytest.raises(ValueError):
        R.box_filter_restate(img, -1, 2, 2, True)
    with pytest.raises(ValueError):
        R.box_filter_restate(img, R.CV_32S, 256, 3, False)
    assert 255 * R.MAX_SIDE * R.MAX_SIDE < 1 << 24            # so CV_32F holds every sum the window sides allow
    assert R.box_filter_restate(img, R.CV_32F, 255, 255, False).dtype == np.float32


def test_integral_equals_cumsum():
    rng = np.random.default_rng(5)
    for shape in ((1, 1), (1, 9), (9, 1), (13, 17), (6, 5, 3), (4, 7, 4)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        got = R.integral_restate(img)
        assert got.dtype == np.int32 and got.shape == (shape[0] + 1, shape[1] + 1) + shape[2:]
        assert not got[0].any() and not got[:, 0].any()
        assert np.array_equal(got[1:, 1:], img.astype(np.int64).cumsum(0).cumsum(1))
    with pytest.raises(ValueError):
        R.integral_restate(np.lib.stride_tricks.as_strided(np.zeros(1, np.uint8), (4000, 4000), (0, 0)))


def test_pyr_down_equals_scipy_mirror_correlation():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(7)
    k2 = np.outer(R.K5, R.K5)
    for shape in ((3, 3), (5, 4), (2, 7), (16, 33), (9, 12, 3)):
        img = rng.integers(0, 256, shape, dtype=np.uint8).astype(np.int64)
        if img.ndim == 2:
            full = ndi.correlate(img, k2, mode="mirror")
        else:
            full = np.stack([ndi.correlate(img[:, :, c], k2, mode="mirror") for c in range(shape[2])], axis=2)
        want = ((full[::2, ::2] + 128) >> 8).astype(np.uint8)
        assert np.array_equal(R.pyr_down_restate(img.astype(np.uint8)), want), shape


def test_pyr_down_of_a_single_pixel_is_the_kernel():
    img = np.zeros((12, 12), np.uint8)
    img[6, 4] = 255
    got = R.pyr_down_restate(img).astype(np.int64)
    # result (y, x) reads source rows 2y - 2 .. 2y + 2: the source pixel (6, 4) is tap 2y - 4 .. of results y = 2, 3, 4 -> taps 4, 2, 0
    taps = {2: 1, 3: 6, 4: 1}
    tapsx = {1: 1, 2: 6, 3: 1}
    want = np.zeros((6, 6), np.int64)
    for y, ky in taps.items():
        for x, kx in tapsx.items():
            want[y, x] = (ky * kx * 255 + 128) >> 8
    assert np.array_equal(got, want)
    odd = np.zeros((12, 12), np.uint8)
    odd[5, 5] = 255                                           # an odd pixel meets the taps 4 and 4
    got = R.pyr_down_restate(odd).astype(np.int64)
    want = np.zeros((6, 6), np.int64)
    want[2:4, 2:4] = (16 * 255 + 128) >> 8
    assert np.array_equal(got, want)


@pytest.mark.parametrize("value", [0, 1, 127, 255])
def test_a_constant_image_stays_constant(value):
    for shape in ((1, 1), (2, 2), (3, 5), (8, 7, 3)):
        img = np.full(shape, value, np.uint8)
        for kw, kh in ((3, 3), (5, 1), (1, 7), (15, 15), (9, 9)):
            for border in (R.BORDER_REFLECT_101, R.BORDER_REPLICATE, R.BORDER_REFLECT):
                assert (R.box_filter_restate(img, -1, kw, kh, True, border) == value).all()
        for border in R.PYR_DOWN_BORDERS:
            assert (R.pyr_down_restate(img, border) == value).all()
        up = R.pyr_up_restate(img)
        assert up.shape == (2 * shape[0], 2 * shape[1]) + shape[2:] and (up == value).all()


def test_pyr_up_known_answers():
    assert np.array_equal(R.pyr_up_restate(np.array([[77]], np.uint8)), np.full((2, 2), 77, np.uint8))
    s = np.array([[10, 200, 30, 40]], np.uint8)
    row = np.array([6 * 10 + 2 * 200, 4 * (10 + 200), 10 + 6 * 200 + 30, 4 * (200 + 30), 200 + 6 * 30 + 40, 4 * (30 + 40), 30 + 7 * 40, 8 * 40], np.int64)
    want = np.stack([(8 * row + 32) >> 6, (8 * row + 32) >> 6]).astype(np.uint8)       # one source row: both result rows are 8 r
    assert np.array_equal(R.pyr_up_restate(s), want)
    assert np.array_equal(R.pyr_up_restate(np.ascontiguousarray(s.T)), want.T)
    two = np.array([[0, 64], [128, 255]], np.uint8).astype(np.int64)
    r = np.stack([np.array([6 * a + 2 * b, 4 * (a + b), a + 7 * b, 8 * b]) for a, b in two])
    want = np.stack([(6 * r[0] + 2 * r[1] + 32) >> 6, (4 * (r[0] + r[1]) + 32) >> 6, (r[0] + 7 * r[1] + 32) >> 6, (8 * r[1] + 32) >> 6]).astype(np.uint8)
    assert np.array_equal(R.pyr_up_restate(two.astype(np.uint8)), want)
    with pytest.raises(ValueError):
        R.pyr_up_restate(s, R.BORDER_REPLICATE)
    with pytest.raises(ValueError):
        R.pyr_down_restate(s, R.BORDER_CONSTANT)
    with pytest.raises(ValueError):
        R.pyr_down_restate(s, R.BORDER_WRAP)


def test_admitted_areas():
    """every odd square up to 151 is admitted, as the proof of test_oracle.py::test_adaptive_threshold_mean_restatement has it; the
    areas refused below 64 are exactly the even ones: each has a sum on an exact tie, which the Q23 reciprocal rounds up and the
    float products round to even"""
    for bs in range(1, 152, 2):
        assert R.area_is_exact(bs * bs), bs
    assert [a for a in range(1, 64) if not R.area_is_exact(a)] == list(range(2, 64, 2))
    for a in (3, 9, 25, 225):                                 # admitted: the common byte is the nearest integer
        s = np.arange(0, 255 * a + 1, dtype=np.int64)
        assert np.array_equal(R._mean(s, a), (2 * s + a) // (2 * a))
    with pytest.raises(ValueError):
        R.area_is_exact(0)
