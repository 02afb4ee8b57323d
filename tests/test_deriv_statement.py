"""CPU suite for the statement of the derivative filters (tests/deriv_restate.py): it equals scipy.ndimage.correlate on int64 for every
operator, kernel size and border; its tap tables are cv::getDerivKernels'; its casts saturate; and its border index maps are
cv::borderInterpolate's also where the image is narrower than the kernel's radius."""
import functools

import numpy as np
import pytest
from scipy import ndimage

import deriv_restate as R

MODES = {R.BORDER_REFLECT_101: "mirror", R.BORDER_REPLICATE: "nearest", R.BORDER_REFLECT: "reflect", R.BORDER_CONSTANT: "constant"}
SOBELS = [(dx, dy, k) for k in (1, 3, 5, 7, -1) for dx in range(3) for dy in range(3)
          if dx + dy > 0 and ((k == -1 and dx + dy == 1) or k == 1 or (k > 1 and max(dx, dy) < k))]


@functools.lru_cache(maxsize=None)
def _images():
    rng = np.random.default_rng(11)
    step = np.zeros((19, 23), np.uint8)
    step[:, 12:] = 255
    hstep = np.ascontiguousarray(step.T)
    return {"random": rng.integers(0, 256, (21, 17), dtype=np.uint8), "step": step, "hstep": hstep,
            "bgr": rng.integers(0, 256, (9, 13, 3), dtype=np.uint8)}


def _scipy(img, k2d, border):
    a = img.astype(np.int64)
    k = np.asarray(k2d, np.int64)
    if a.ndim == 2:
        return ndimage.correlate(a, k, mode=MODES[border], cval=0)
    return np.stack([ndimage.correlate(a[:, :, c], k, mode=MODES[border], cval=0) for c in range(a.shape[2])], axis=2)


@pytest.mark.parametrize("border", sorted(MODES))
def test_statement_equals_scipy_correlate_for_every_operator_and_ksize(border):
    for name, img in _images().items():
        for dx, dy, k in SOBELS:
            ky, kx = R.sobel_kernel(dx, dy, k)
            k2d = np.outer(ky, kx)
            want = _scipy(img, k2d, border)
            assert np.array_equal(R.correlate(img, k2d, border), want), (name, dx, dy, k)
            for dd in (R.CV_8U, R.CV_16S, R.CV_32F, R.CV_64F):
                got = R.sobel_restate(img, dd, dx, dy, k, border)
                assert got.dtype == R.DTYPES[dd] and np.array_equal(got, R.saturate(want, dd)), (name, dx, dy, k, dd)
        for dx, dy in ((1, 0), (0, 1)):
            ky, kx = R.scharr_kernel(dx, dy)
            assert np.array_equal(R.scharr_restate(img, R.CV_32F, dx, dy, border), _scipy(img, np.outer(ky, kx), border).astype(np.float32))
        for k in (1, 3, 5, 7):
            want = _scipy(img, R.laplacian_kernel(k), border)
            assert np.array_equal(R.laplacian_restate(img, R.CV_64F, k, border), want.astype(np.float64)), (name, k)
            sob = R.correlate(img, np.outer(*R.sobel_kernel(2, 0, max(k, 3))), border) + R.correlate(img, np.outer(*R.sobel_kernel(0, 2, max(k, 3))), border)
            if k >= 3:
                assert np.array_equal(want, sob), "Laplacian = Sobel(2,0) + Sobel(0,2)"
        if img.ndim == 2 and border in (R.BORDER_REFLECT_101, R.BORDER_REPLICATE):
            gx, gy = R.spatial_gradient_restate(img, border)
            assert np.array_equal(gx, R.saturate(_scipy(img, [[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], border), R.CV_16S))
            assert np.array_equal(gy, R.saturate(_scipy(img, [[-1, -2, -1], [0, 0, 0], [1, 2, 1]], border), R.CV_16S))


def test_tap_tables_are_getderivkernels():
    t = R.deriv_taps
    assert t(3, 0).tolist() == [1, 2, 1] and t(3, 1).tolist() == [-1, 0, 1] and t(3, 2).tolist() == [1, -2, 1]
    assert t(5, 0).tolist() == [1, 4, 6, 4, 1] and t(5, 1).tolist() == [-1, -2, 0, 2, 1] and t(5, 2).tolist() == [1, 0, -2, 0, 1]
    assert t(7, 0).tolist() == [1, 6, 15, 20, 15, 6, 1] and t(7, 1).tolist() == [-1, -4, -5, 0, 5, 4, 1] and t(7, 2).tolist() == [1, 2, -1, -4, -1, 2, 1]
    assert t(1, 0).tolist() == [1]
    ky, kx = R.sobel_kernel(1, 0, 1)
    assert ky.tolist() == [1] and kx.tolist() == [-1, 0, 1]
    ky, kx = R.sobel_kernel(0, 2, 1)
    assert ky.tolist() == [1, -2, 1] and kx.tolist() == [1]
    ky, kx = R.sobel_kernel(1, 0, -1)
    assert ky.tolist() == [3, 10, 3] and kx.tolist() == [-1, 0, 1]
    assert R.laplacian_kernel(1).tolist() == [[0, 1, 0], [1, -4, 1], [0, 1, 0]] and R.laplacian_kernel(3).tolist() == [[2, 0, 2], [0, -8, 0], [2, 0, 2]]
    # the bounds the kernels and the statement's docstring rest on
    assert max(np.abs(t(k, o)).sum() for k in (3, 5, 7) for o in range(3)) * 255 == 16320
    assert np.abs(t(5, 2)).sum() * np.abs(t(5, 0)).sum() * 255 <= 32767, "each Laplacian term at 5 stays inside int16"


def test_int16_saturates_and_uint8_clamps_negatives():
    step = _images()["step"]
    raw = R.correlate(step, np.outer(*R.sobel_kernel(1, 0, 7)), R.BORDER_REFLECT_101)
    assert raw.max() > 150000 and raw.min() == 0
    neg = R.correlate(np.ascontiguousarray(step[:, ::-1]), np.outer(*R.sobel_kernel(1, 0, 7)), R.BORDER_REFLECT_101)
    assert neg.min() < -150000
    s = R.sobel_restate(step, R.CV_16S, 1, 0, 7)
    assert s.dtype == np.int16 and s.max() == 32767 and s.min() == 0
    s = R.sobel_restate(np.ascontiguousarray(step[:, ::-1]), R.CV_16S, 1, 0, 7)
    assert s.min() == -32768 and s.max() == 0
    u = R.sobel_restate(np.ascontiguousarray(step[:, ::-1]), R.CV_8U, 1, 0, 3)
    assert u.dtype == np.uint8 and u.max() == 0, "negative responses clamp to 0"
    u = R.sobel_restate(step, -1, 1, 0, 3)
    assert u.max() == 255 and set(np.unique(u)) == {0, 255}
    f = R.sobel_restate(step, R.CV_32F, 1, 0, 7)
    assert f.dtype == np.float32 and np.array_equal(f.astype(np.int64), raw), "float32 holds the integer exactly"


def _periodic(p, n, border):
    """the closed forms of the three index maps, written independently of borderInterpolate's loop"""
    if border == R.BORDER_REPLICATE:
        return min(max(p, 0), n - 1)
    if border == R.BORDER_REFLECT:
        q = p % (2 * n)
        return q if q < n else 2 * n - 1 - q
    if n == 1:
        return 0
    q = p % (2 * n - 2)
    return q if q < n else 2 * n - 2 - q


def test_border_maps_follow_borderinterpolate_also_on_narrow_images():
    for n in (1, 2, 3, 4, 9):
        for border in (R.BORDER_REPLICATE, R.BORDER_REFLECT, R.BORDER_REFLECT_101):
            for p in range(-12, n + 12):
                assert R.border_index(p, n, border) == _periodic(p, n, border), (n, border, p)
        for p in range(-12, n + 12):
            assert R.border_index(p, n, R.BORDER_CONSTANT) == (p if 0 <= p < n else -1)
    # cv2's documented examples: gfedcb|abcdefgh|gfedcba and fedcba|abcdefgh|hgfedcb
    assert [R.border_index(p, 8, R.BORDER_REFLECT_101) for p in (-2, -1, 8, 9)] == [2, 1, 6, 5]
    assert [R.border_index(p, 8, R.BORDER_REFLECT) for p in (-2, -1, 8, 9)] == [1, 0, 7, 6]
    rng = np.random.default_rng(3)
    for h, w in ((1, 1), (1, 9), (9, 1), (2, 2), (3, 5), (2, 7), (7, 3)):
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        for border in sorted(MODES):
            k2d = np.outer(*R.sobel_kernel(1, 0, 7))
            ext = R.extend(img, 3, 3, border)
            for y in range(-3, h + 3):
                for x in range(-3, w + 3):
                    if border == R.BORDER_CONSTANT:
                        want = int(img[y, x]) if (0 <= y < h and 0 <= x < w) else 0
                    else:
                        want = int(img[_periodic(y, h, border), _periodic(x, w, border)])
                    assert ext[y + 3, x + 3] == want, (h, w, border, y, x)
            assert R.correlate(img, k2d, border).shape == (h, w)


def test_convert_scale_abs_statement():
    v = np.array([-32768, -32767, -256, -255, -254, -1, 0, 1, 254, 255, 256, 32767], np.int16)
    assert R.convert_scale_abs_restate(v).tolist() == [255, 255, 255, 255, 254, 1, 0, 1, 254, 255, 255, 255]
    f = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 254.5, 255.5, -254.5, 253.5, 1e9, -1e9, np.inf, -np.inf, np.nan, 0.49999997, 2.4999998], np.float32)
    assert R.convert_scale_abs_restate(f).tolist() == [0, 2, 2, 0, 2, 2, 254, 255, 254, 254, 255, 255, 255, 255, 0, 0, 2]
    assert R.convert_scale_abs_restate(f.astype(np.float64)).tolist() == R.convert_scale_abs_restate(f).tolist()
    u = np.arange(256, dtype=np.uint8)
    assert np.array_equal(R.convert_scale_abs_restate(u), u)
