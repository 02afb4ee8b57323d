"""CPU suite for the two numpy statements of the median filter (tests/median_restate.py): they agree with each other, with a
triple-loop brute force where the clamp covers most of the window, and with scipy where scipy is importable."""
import numpy as np
import pytest

from median_restate import majority_restate, median_restate

KS = (1, 3, 5, 9, 15)


def _brute(img, k):
    h, w = img.shape
    r = k // 2
    out = np.empty_like(img)
    for y in range(h):
        for x in range(w):
            vals = []
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    vals.append(int(img[min(max(y + dy, 0), h - 1), min(max(x + dx, 0), w - 1)]))
            out[y, x] = sorted(vals)[k * k // 2]
    return out


def test_the_two_statements_agree_on_masks():
    rng = np.random.default_rng(1)
    for (h, w) in ((1, 1), (5, 4), (37, 29), (64, 128)):
        for dens in (0.02, 0.1, 0.5, 0.98):
            m = np.where(rng.random((h, w)) < dens, 255, 0).astype(np.uint8)
            for k in (1, 3, 5, 7, 15, 31, 63):
                assert np.array_equal(median_restate(m, k), majority_restate(m, k)), (h, w, dens, k)


def test_median_restate_equals_brute_force_where_the_clamp_dominates():
    rng = np.random.default_rng(2)
    for (h, w) in ((1, 1), (1, 6), (5, 1), (2, 3), (5, 4), (6, 5)):
        for img in (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.choice(np.array([0, 1, 254, 255], np.uint8), (h, w))):
            for k in KS:
                assert np.array_equal(median_restate(img, k), _brute(img, k)), (h, w, k)
    img = rng.integers(0, 256, (6, 5, 3), dtype=np.uint8)
    for k in KS:
        got = median_restate(img, k)
        assert got.shape == img.shape and got.dtype == np.uint8
        for c in range(3):
            assert np.array_equal(got[:, :, c], _brute(np.ascontiguousarray(img[:, :, c]), k))


def test_median_restate_equals_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    for (h, w) in ((1, 7), (5, 4), (37, 29), (77, 100)):
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        for k in (1, 3, 5, 7, 15, 31):
            assert np.array_equal(median_restate(img, k), ndi.median_filter(img, size=k, mode="nearest")), (h, w, k)


def test_constant_image_is_a_fixed_point_and_k1_is_the_identity():
    rng = np.random.default_rng(4)
    for v in (0, 7, 255):
        for shape in ((9, 6), (4, 5, 3)):
            img = np.full(shape, v, np.uint8)
            for k in (1, 3, 5, 15, 255):
                assert np.array_equal(median_restate(img, k), img)
    m = np.full((9, 6), 255, np.uint8)
    assert np.array_equal(majority_restate(m, 255), m) and not majority_restate(np.zeros((9, 6), np.uint8), 255).any()
    for shape in ((1, 1), (37, 29), (5, 4, 4)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        assert np.array_equal(median_restate(img, 1), img)
    mk = np.where(rng.random((17, 13)) < 0.5, 255, 0).astype(np.uint8)
    assert np.array_equal(majority_restate(mk, 1), mk)
