"""CPU suite for the surface of cv2.boxFilter / blur, pyrDown, pyrUp and integral: the nine C entries are exported by libvp.so and
declared in include/vp.h with the prototypes vision/_vp.py binds; the three kernel sources are built; the codes are cv2's and agree
between header, binding and facade; the facade has cv2's parameter order; the area admission of the library equals the statement's;
the entries without a context fail as their neighbours do and write nothing."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import box_pyr_restate as R
from abi_header import _header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vp_box_filter_u8", "vp_box_filter_dev", "vp_pyr_down_u8", "vp_pyr_down_dev", "vp_pyr_up_u8", "vp_pyr_up_dev", "vp_integral_u8", "vp_integral_dev"]


def test_box_pyr_symbols_are_exported_declared_and_bound_alike():
    from vision import _vp
    protos = _header_prototypes()
    lib = C.CDLL(_vp.LIB_PATH)
    for name in NEW:      # that each is bound as declared: test_abi.py::test_every_prototype_is_bound_as_declared
        assert hasattr(lib, name) and name in protos and name in _vp._SIGS, name
    assert hasattr(lib, "vp_box_area_exact") and protos["vp_box_area_exact"] == ("int", [C.c_int]) and _vp._SIGS["vp_box_area_exact"] == (C.c_int, [C.c_int])
    built = open(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "build.py")).read()
    for src in ("vp_box.hip", "vp_pyr.hip", "vp_integral.hip"):
        assert f'"{src}"' in built, f"{src} is not among VP_SOURCES"


def test_codes_are_cv2s_and_agree_between_header_binding_and_facade():
    from vision import _vp
    from vision import cv2_facade as f
    txt = open(os.path.join(ROOT, "include", "vp.h")).read()

    def code(name):
        m = re.search(r"\b" + name + r"\s*=\s*(-?\d+)", txt)
        assert m, name
        return int(m.group(1))
    assert code("VP_DEPTH_32S") == _vp.DEPTH_32S == f.CV_32S == R.CV_32S == 4
    assert (code("VP_DEPTH_8U"), code("VP_DEPTH_16S"), code("VP_DEPTH_32F"), code("VP_DEPTH_64F")) == (f.CV_8U, f.CV_16S, f.CV_32F, f.CV_64F) == (0, 3, 5, 6)
    assert (code("VP_BORDER_CONSTANT"), code("VP_BORDER_REPLICATE"), code("VP_BORDER_REFLECT"), code("VP_BORDER_REFLECT_101")) == \
        (f.BORDER_CONSTANT, f.BORDER_REPLICATE, f.BORDER_REFLECT, f.BORDER_REFLECT_101) == (R.BORDER_CONSTANT, R.BORDER_REPLICATE, R.BORDER_REFLECT, R.BORDER_REFLECT_101)
    assert f.BORDER_DEFAULT == R.BORDER_REFLECT_101 == 4
    plan = open(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc", "vp_box_plan.h")).read()
    num = lambda n: int(re.search(r"#define " + n + r" (\d+)", plan).group(1))
    assert num("BX_TB") == 256 and num("BX_CHUNK") % 12 == 0 and num("BX_ROW_CHUNK") % 12 == 0 and num("BX_MAXK") == R.MAX_SIDE
    assert num("BX_LDS_BYTES") <= 64 * 1024 and num("IG_SCAN") == 64 * num("IG_CHUNK")
    assert num("PD_TW") % 4 == 0 and num("PU_TW") % 2 == 0 and min(num("PD_TH"), num("PU_TH"), num("BX_TH"), num("BX_STRIP")) >= 1


def test_facade_has_cv2s_parameter_order_and_the_mirror_has_the_names():
    from vision import cv2_facade as f
    from vision.utils import transform
    sig = lambda fn: list(inspect.signature(fn).parameters)
    assert sig(f.blur) == ["src", "ksize", "dst", "anchor", "borderType"]
    assert sig(f.boxFilter) == ["src", "ddepth", "ksize", "dst", "anchor", "normalize", "borderType"]
    assert sig(f.pyrDown) == sig(f.pyrUp) == ["src", "dst", "dstsize", "borderType"]
    assert sig(f.buildPyramid)[:2] == ["src", "maxlevel"]
    assert sig(f.integral) == ["src", "sum", "sdepth"]
    p = inspect.signature(f.boxFilter).parameters
    assert p["anchor"].default == (-1, -1) and p["normalize"].default is True and p["borderType"].default == f.BORDER_DEFAULT
    assert inspect.signature(f.integral).parameters["sdepth"].default == -1
    assert sig(transform.box_blur) == ["mat", "kx", "ky"] and sig(transform.box_filter)[:3] == ["mat", "kx", "ky"]
    assert sig(transform.pyr_down)[0] == sig(transform.pyr_up)[0] == sig(transform.integral)[0] == "mat"
    assert sig(transform.build_pyramid) == ["mat", "levels"]


def test_facade_refuses_before_it_needs_a_device():
    """what cv2 or this path rejects is cv2.error, raised from the arguments alone"""
    import pytest
    from vision import cv2_facade as f
    img = np.zeros((6, 5), np.uint8)
    for call in (lambda: f.blur(img, (2, 2)), lambda: f.blur(img, (3, 3), None, (0, 0)), lambda: f.blur(img.astype(np.float32), (3, 3)),
                 lambda: f.boxFilter(img, f.CV_16S, (3, 3)), lambda: f.boxFilter(img, 2, (3, 3), normalize=False), lambda: f.blur(img, (3, 3), borderType=f.BORDER_WRAP),
                 lambda: f.blur(img, (256, 3)), lambda: f.pyrDown(img, None, (2, 2)), lambda: f.pyrUp(img, None, (5, 6)), lambda: f.pyrDown(img, borderType=f.BORDER_CONSTANT),
                 lambda: f.pyrUp(img, borderType=f.BORDER_REPLICATE), lambda: f.integral(img, None, f.CV_64F), lambda: f.integral(img.astype(np.int16)),
                 lambda: f.integral2(img), lambda: f.integral3(img), lambda: f.buildPyramid(img, -1)):
        with pytest.raises(f.error):
            call()


def test_area_admission_of_the_library_equals_the_statement():
    from vision import _vp
    lib = C.CDLL(_vp.LIB_PATH)
    lib.vp_box_area_exact.restype, lib.vp_box_area_exact.argtypes = C.c_int, [C.c_int]
    for area in list(range(1, 401)) + [1023, 1024, 1025, 51 * 51, 4 * 1000, 101 * 77, 150 * 151, 151 * 151]:
        assert lib.vp_box_area_exact(area) == int(R.area_is_exact(area)), area
    assert lib.vp_box_area_exact(0) < 0 and lib.vp_box_area_exact(-3) < 0
    assert lib.vp_box_area_exact(9) == 1                       # (the second call answers from the cache)


def test_entries_without_a_context_fail_like_their_neighbours_and_write_nothing():
    from vision import _vp
    lib = C.CDLL(_vp.LIB_PATH)
    for name in NEW + ["vp_deriv_u8"]:
        res, args = _vp._SIGS[name]
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    src = np.arange(30, dtype=np.uint8).reshape(6, 5)
    dst = np.full((14, 12), 77, np.int32)
    p = lambda a: a.ctypes.data
    ref = lib.vp_deriv_u8(None, p(src), 5, 6, 1, 0, 1, 0, 3, 3, 4, p(dst))
    assert ref == _vp.ERR_INVALID
    assert lib.vp_box_filter_u8(None, p(src), 5, 6, 1, 3, 3, 1, -1, 4, p(dst)) == ref
    assert lib.vp_box_filter_dev(None, p(src), 5, 5, 6, 1, 3, 3, 0, 4, 4, p(dst)) == ref
    assert lib.vp_pyr_down_u8(None, p(src), 5, 6, 1, 4, p(dst)) == ref
    assert lib.vp_pyr_down_dev(None, p(src), 5, 5, 6, 1, 4, p(dst)) == ref
    assert lib.vp_pyr_up_u8(None, p(src), 5, 6, 1, p(dst)) == ref
    assert lib.vp_pyr_up_dev(None, p(src), 5, 5, 6, 1, p(dst)) == ref
    assert lib.vp_integral_u8(None, p(src), 5, 6, 1, p(dst)) == ref
    assert lib.vp_integral_dev(None, p(src), 5, 5, 6, 1, p(dst)) == ref
    assert (dst == 77).all(), "a destination was written without a context"
