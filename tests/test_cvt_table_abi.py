"""CPU suite for the added conversion codes: vision/_vp.py carries the values of include/vp.h, the channel table of the mirror agrees
with the header's grouping, and every new code is turned away cleanly (no crash) when the context is NULL."""
import ctypes as C
import os
import re

import numpy as np

NEW = ["BGR2YUV", "YUV2BGR", "YCRCB2BGR", "BGR2XYZ", "XYZ2BGR", "HLS2BGR", "BGR2RGB", "RGB2GRAY", "RGB2HSV", "HSV2RGB", "RGB2HLS", "HLS2RGB",
       "RGB2LAB", "LAB2RGB", "RGB2YCRCB", "YCRCB2RGB", "RGB2YUV", "YUV2RGB", "RGB2XYZ", "XYZ2RGB", "BGRA2BGR", "RGBA2BGR", "BGR2BGRA",
       "BGR2RGBA", "BGRA2RGBA", "GRAY2BGRA", "BGRA2GRAY", "RGBA2GRAY"]
OLD = {"BGR2LAB": 0, "BGR2HSV": 1, "BGR2GRAY": 2, "GRAY2BGR": 3, "HSV2BGR": 4, "BGR2YCRCB": 5, "BGR2HLS": 6, "LAB2BGR": 7}


def _header():
    return open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vp.h")).read()


def test_constants_equal_the_header():
    from vision import _vp
    txt = _header()
    seen = set()
    for name in list(OLD) + NEW:
        m = re.search(r"\bVP_" + name + r"\s*=\s*(\d+)", txt)
        assert m, name
        assert getattr(_vp, name) == int(m.group(1)), name
        seen.add(int(m.group(1)))
    for name, value in OLD.items():
        assert getattr(_vp, name) == value, f"{name} moved"
    assert seen == set(range(len(OLD) + len(NEW))), "the codes are not dense"
    m = re.search(r"\bVP_CVT_CODES\s*=\s*(\d+)", txt)
    assert m and int(m.group(1)) == _vp.CVT_CODES == len(OLD) + len(NEW)
    assert _vp.CVT_CODES <= 99      # tests/test_gpu_parity.py passes 99 as an unknown code


def test_channel_table_follows_the_names():
    from vision import _vp
    cn = {"GRAY": 1, "BGRA": 4, "RGBA": 4}
    for name in list(OLD) + NEW:
        src, dst = name.split("2")
        assert _vp.CVT_CHANNELS.get(getattr(_vp, name), (3, 3)) == (cn.get(src, 3), cn.get(dst, 3)), name


def test_every_new_code_is_rejected_without_a_context():
    from vision import _vp
    lib = C.CDLL(_vp.LIB_PATH)
    for fn in (lib.vp_cvt_color_u8, lib.vp_cvt_color_dev):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    src = np.zeros((4, 4, 4), np.uint8)
    dst = np.zeros((4, 4, 4), np.uint8)
    for name in NEW:
        code = getattr(_vp, name)
        assert lib.vp_cvt_color_u8(None, code, src.ctypes.data, 16, 4, 4, dst.ctypes.data, None) < 0, name
        assert lib.vp_cvt_color_dev(None, code, src.ctypes.data, 16, 4, 4, dst.ctypes.data, None) < 0, name
    assert not dst.any()


def test_facade_names_carry_cv2s_values():
    from vision import cv2_facade as f
    values = {"BGR2BGRA": 0, "BGRA2BGR": 1, "RGBA2RGB": 1, "BGR2RGBA": 2, "RGBA2BGR": 3, "BGRA2RGB": 3, "BGR2RGB": 4, "RGB2BGR": 4, "BGRA2RGBA": 5,
              "RGBA2BGRA": 5, "RGB2GRAY": 7, "GRAY2BGRA": 9, "BGRA2GRAY": 10, "RGBA2GRAY": 11, "BGR2XYZ": 32, "RGB2XYZ": 33, "XYZ2BGR": 34,
              "XYZ2RGB": 35, "RGB2YCrCb": 37, "RGB2YCR_CB": 37, "YCrCb2BGR": 38, "YCR_CB2BGR": 38, "YCrCb2RGB": 39, "YCR_CB2RGB": 39, "RGB2HSV": 41,
              "RGB2Lab": 45, "RGB2LAB": 45, "RGB2HLS": 53, "HSV2RGB": 55, "Lab2RGB": 57, "LAB2RGB": 57, "HLS2BGR": 60, "HLS2RGB": 61, "BGR2YUV": 82,
              "RGB2YUV": 83, "YUV2BGR": 84, "YUV2RGB": 85}
    for name, value in values.items():
        assert getattr(f, "COLOR_" + name) == value, name
        assert value in f._CVT, name
    assert f.COLOR_BGR2LUV not in f._CVT
    from vision.utils import color
    for name in ("bgr_to_yuv", "yuv_to_bgr", "bgr_to_xyz", "xyz_to_bgr", "ycrcb_to_bgr", "hls_to_bgr"):
        assert callable(getattr(color, name)), name
