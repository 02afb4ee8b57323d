"""CPU suite for the median filter's surface: both C entries are exported by libvp.so and declared in include/vp.h with the prototypes
vision/_vp.py binds; cv2_facade.medianBlur has cv2's parameter order and rejects what is outside the path before anything is
launched; the host entry without a context answers as the blur entries do and writes nothing."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from abi_header import _header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vp_median_blur_u8", "vp_median_blur_dev"]


def test_median_symbols_are_exported_declared_and_bound_alike():
    from vision import _vp
    protos = _header_prototypes()
    lib = C.CDLL(_vp.LIB_PATH)
    for name in NEW:      # that each is bound as declared: test_abi.py::test_every_prototype_is_bound_as_declared
        assert hasattr(lib, name) and name in protos and name in _vp._SIGS, name
    built = open(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "build.py")).read()
    assert '"vp_median.hip"' in built, "vp_median.hip is not among VP_SOURCES"


def test_median_options_are_declared_and_bound():
    from vision import _vp
    txt = open(os.path.join(ROOT, "include", "vp.h")).read()
    for name, value in (("VP_OPT_MEDIAN_MASK", _vp.OPT_MEDIAN_MASK),):
        m = re.search(name + r"\s*=\s*(\d+)", txt)
        assert m and int(m.group(1)) == value
        assert txt.count(name) >= 2, "the option is documented with the others"


def test_medianblur_has_cv2s_parameter_order_and_the_mirror_has_the_name():
    from vision import cv2_facade as f
    from vision.utils import transform
    assert list(inspect.signature(f.medianBlur).parameters) == ["src", "ksize", "dst"]
    assert list(inspect.signature(transform.median_blur).parameters) == ["mat", "ksize"]


def test_medianblur_rejects_what_is_outside_the_path():
    from vision import cv2_facade as f
    g = np.zeros((6, 5), np.uint8)
    bad = [(g, 4), (g, 0), (g, -3), (g, 2),                                 # even or non-positive
           (g, 257), (g, 1001),                                             # outside the accelerated path
           (np.zeros((6, 5), np.float32), 3), (np.zeros((6, 5), np.uint16), 3), (np.zeros((6, 5, 3), np.int8), 5),   # not uint8
           (np.zeros((0, 5), np.uint8), 3), (np.zeros((6, 0, 3), np.uint8), 3),                                      # empty
           (np.zeros((6, 5, 5), np.uint8), 3),                              # more than 4 channels
           (np.zeros((6, 5, 2), np.uint8), 7), (np.zeros((6, 5, 2), np.uint8), 31)]                                 # 2 channels above 5
    for src, k in bad:
        with pytest.raises(f.error):
            f.medianBlur(src, k)
    with pytest.raises(f.error) as e:
        f.medianBlur(g, 257)
    assert "outside the accelerated path" in str(e.value)
    from vision.utils.transform import median_blur
    for k in (0, 4, 257):
        with pytest.raises(ValueError):
            median_blur(g, k)
    with pytest.raises(TypeError):
        median_blur(np.zeros((6, 5), np.float32), 3)


def test_host_entry_without_a_context_answers_like_the_blur_and_writes_nothing():
    from vision import _vp
    lib = C.CDLL(_vp.LIB_PATH)
    for name in ("vp_median_blur_u8", "vp_gaussian_blur_u8", "vp_median_blur_dev"):
        res, args = _vp._SIGS[name]
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    src = np.arange(30, dtype=np.uint8).reshape(6, 5)
    dst = np.full((6, 5), 77, np.uint8)
    blur = lib.vp_gaussian_blur_u8(None, src.ctypes.data, 5, 6, 1, 3, 3, 0.0, 0.0, dst.ctypes.data)
    assert blur == _vp.ERR_INVALID and (dst == 77).all()
    assert lib.vp_median_blur_u8(None, src.ctypes.data, 5, 6, 1, 3, dst.ctypes.data) == blur
    assert (dst == 77).all(), "the destination was written without a context"
    made = C.c_int(-5)
    assert lib.vp_median_blur_dev(None, src.ctypes.data, 5, 5, 6, 1, 3, 0, None, dst.ctypes.data, None, C.byref(made)) == blur
    assert made.value == -5 and (dst == 77).all()
