"""CPU suite for the device-resident blur / resize / warp / threshold / histogram / labelling entries: every new symbol is exported by
libvp.so and declared in include/vp.h with the prototype vision/_vp.py binds; the histogram statistics simple_canny uses for a device
image equal numpy's bit for bit; cv2_facade.threshold exists, rejects what cv2 rejects and has no CPU path."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from abi_header import _header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["vp_gaussian_blur_dev", "vp_resize_dev", "vp_warp_affine_dev", "vp_threshold_u8_dev", "vp_otsu_threshold_dev",
       "vp_adaptive_threshold_mean_dev", "vp_hist_u8_dev", "vp_ccl_dev", "vp_ccl_bits_dev"]


def test_new_symbols_are_exported_declared_and_bound_alike():
    from vision import _vp
    protos = _header_prototypes()
    lib = C.CDLL(_vp.LIB_PATH)
    for name in NEW:      # that each is bound as declared: test_abi.py::test_every_prototype_is_bound_as_declared
        assert hasattr(lib, name) and name in protos and name in _vp._SIGS, name


def test_blur_onepass_option_is_declared():
    from vision import _vp
    txt = open(os.path.join(ROOT, "include", "vp.h")).read()
    m = re.search(r"VP_OPT_BLUR_ONEPASS\s*=\s*(\d+)", txt)
    assert m and int(m.group(1)) == _vp.OPT_BLUR_ONEPASS
    assert txt.count("VP_OPT_BLUR_ONEPASS") >= 2, "the option is documented with the others"


def _counts(a):
    return np.bincount(np.asarray(a, np.uint8).ravel(), minlength=256)


def _same_bits(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def test_histogram_median_and_mean_equal_numpy():
    from vision.utils.feature import hist_mean, hist_median
    rng = np.random.default_rng(20)
    arrays = [rng.integers(0, 256, n, dtype=np.uint8) for n in (1, 2, 3, 4, 7, 8, 101, 1000, 1001, 4096, 99991)]
    arrays += [rng.integers(0, 256, (37, 41, 3), dtype=np.uint8), rng.integers(0, 256, (36, 41, 3), dtype=np.uint8),
               rng.integers(100, 103, (64, 64), dtype=np.uint8), rng.integers(0, 2, 999, dtype=np.uint8) * 255]
    arrays += [np.full(9, 7, np.uint8), np.full(10, 255, np.uint8), np.zeros(5, np.uint8), np.array([0], np.uint8), np.array([255], np.uint8)]
    arrays += [np.array([10, 200] * 6, np.uint8), np.array([10, 200] * 6 + [200], np.uint8), np.array([10, 11], np.uint8),
               np.array([0, 255], np.uint8), np.array([3, 3, 4, 4], np.uint8), np.array([3, 4, 4, 4], np.uint8)]
    for a in arrays:
        c = _counts(a)
        assert _same_bits(hist_median(c), np.median(a)), (a.shape, hist_median(c), np.median(a))
        assert _same_bits(hist_mean(c), np.mean(a)), (a.shape, hist_mean(c), np.mean(a))
    # a frame's worth of one value and of two: sums far above 2^32 stay exact
    big = np.zeros(256, np.int64)
    big[255] = 3840 * 2160 * 3
    assert hist_mean(big) == 255.0 and hist_median(big) == 255.0
    big[254] = big[255]
    assert hist_mean(big) == 254.5 and hist_median(big) == 254.5
    big[254] += 1
    assert hist_median(big) == 254.0
    with pytest.raises(ValueError):
        hist_median(np.zeros(256, np.int64))
    with pytest.raises(ValueError):
        hist_mean(np.zeros(256, np.int64))


def test_facade_threshold_exists_and_rejects_what_cv2_rejects():
    from vision import _vp
    from vision import cv2_facade as f
    assert (f.THRESH_BINARY, f.THRESH_BINARY_INV, f.THRESH_TRUNC, f.THRESH_TOZERO, f.THRESH_TOZERO_INV, f.THRESH_OTSU) == (0, 1, 2, 3, 4, 8)
    import inspect
    assert list(inspect.signature(f.threshold).parameters)[:4] == ["src", "thresh", "maxval", "type"]
    g = np.zeros((6, 5), np.uint8)
    bad = [(np.zeros((6, 5), np.float32), 1, 255, f.THRESH_BINARY),              # not 8-bit on this path
           (np.zeros((0, 5), np.uint8), 1, 255, f.THRESH_BINARY),                 # empty
           ([[1, 2]], 1, 255, f.THRESH_BINARY),                                    # not an image
           (g, 1, 255, 5), (g, 1, 255, 7), (g, 1, 255, 32), (g, 1, 255, -1),      # unknown types
           (g, 1, 255, f.THRESH_BINARY | 16),                                      # THRESH_TRIANGLE: not offered
           (np.zeros((6, 5, 3), np.uint8), 0, 255, f.THRESH_BINARY | f.THRESH_OTSU),   # Otsu needs CV_8UC1
           (g, float("nan"), 255, f.THRESH_BINARY)]
    for args in bad:
        with pytest.raises(f.error):
            f.threshold(*args)
    import torch
    if not torch.cuda.is_available():                     # no device: the call itself fails loudly, as every operator does
        for kind in (f.THRESH_BINARY, f.THRESH_TRUNC, f.THRESH_TOZERO_INV, f.THRESH_BINARY | f.THRESH_OTSU):
            with pytest.raises(_vp.VpError):
                f.threshold(g, 10, 255, kind)
