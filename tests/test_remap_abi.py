"""CPU suite for the surface of cv2.remap / convertMaps / warpPerspective: the six C entries are exported by libvp.so and declared in
include/vp.h with the prototypes vision/_vp.py binds; the codes are cv2's and agree between header, binding and facade; the facade
has cv2's parameter order; the entries without a context fail as their neighbours do and write nothing."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from abi_header import _header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vp_convert_maps_dev", "vp_remap_fixed_dev", "vp_remap_f32_dev", "vp_remap_u8", "vp_warp_perspective_u8", "vp_warp_perspective_dev"]


def test_remap_symbols_are_exported_declared_and_bound_alike():
    from vision import _vp
    protos = _header_prototypes()
    lib = C.CDLL(_vp.LIB_PATH)
    for name in NEW:      # that each is bound as declared: test_abi.py::test_every_prototype_is_bound_as_declared
        assert hasattr(lib, name) and name in protos and name in _vp._SIGS, name
    built = open(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "build.py")).read()
    assert '"vp_remap.hip"' in built, "vp_remap.hip is not among VP_SOURCES"


def test_codes_are_cv2s_and_agree_between_header_binding_and_facade():
    from vision import _vp
    from vision import cv2_facade as f
    txt = open(os.path.join(ROOT, "include", "vp.h")).read()

    def code(name):
        m = re.search(r"\b" + name + r"\s*=\s*(-?\d+)", txt)
        assert m, name
        return int(m.group(1))
    assert (code("VP_INTER_NEAREST"), code("VP_INTER_LINEAR")) == (_vp.INTER_NEAREST, _vp.INTER_LINEAR) == (f.INTER_NEAREST, f.INTER_LINEAR) == (0, 1)
    assert code("VP_WARP_INVERSE_MAP") == _vp.WARP_INVERSE_MAP == f.WARP_INVERSE_MAP == 16
    assert (code("VP_BORDER_CONSTANT"), code("VP_BORDER_REPLICATE")) == (f.BORDER_CONSTANT, f.BORDER_REPLICATE) == (0, 1)
    assert (f.CV_16UC1, f.CV_32FC1, f.CV_16SC2, f.CV_32FC2) == (2, 5, 11, 13)
    plan = open(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc", "vp_remap_plan.h")).read()
    num = lambda n: int(re.search(r"#define " + n + r" (\d+)", plan).group(1))
    assert num("RM_TW") == 64 * num("RM_PPT") and num("RM_TH") * 64 == 256 and num("RM_MAX_SRC") == 32767


def test_facade_has_cv2s_parameter_order_and_the_mirror_has_the_names():
    from vision import cv2_facade as f
    from vision.utils import transform
    sig = lambda fn: list(inspect.signature(fn).parameters)
    assert sig(f.remap) == ["src", "map1", "map2", "interpolation", "dst", "borderMode", "borderValue"]
    assert sig(f.warpPerspective) == ["src", "M", "dsize", "dst", "flags", "borderMode", "borderValue"]
    assert sig(f.convertMaps) == ["map1", "map2", "dstmap1type", "nninterpolation"]
    assert sig(f.undistort) == ["src", "cameraMatrix", "distCoeffs", "dst", "newCameraMatrix"]
    assert sig(f.initUndistortRectifyMap) == ["cameraMatrix", "distCoeffs", "R", "newCameraMatrix", "size", "m1type"]
    assert sig(f.getPerspectiveTransform)[:2] == ["src", "dst"] and sig(f.perspectiveTransform)[:2] == ["src", "m"]
    p = inspect.signature(f.warpPerspective).parameters
    assert p["flags"].default == f.INTER_LINEAR and p["borderMode"].default == f.BORDER_CONSTANT and p["borderValue"].default == 0
    assert sig(transform.remap)[:4] == ["mat", "map_x", "map_y", "nearest"] and inspect.signature(transform.remap).parameters["nearest"].default is False
    assert sig(transform.warp_perspective) == ["mat", "M", "width", "height"]
    assert sig(transform.undistorter) == ["camera_matrix", "dist_coeffs", "size", "new_camera_matrix"]
    assert hasattr(transform.RemapTable, "apply")


def test_entries_without_a_context_fail_like_their_neighbours_and_write_nothing():
    from vision import _vp
    lib = C.CDLL(_vp.LIB_PATH)
    for name in NEW + ["vp_warp_affine_u8"]:
        res, args = _vp._SIGS[name]
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    src = np.arange(30, dtype=np.uint8).reshape(6, 5)
    dst = np.full((6, 5), 77, np.uint8)
    mx = np.zeros((6, 5), np.float32)
    xy = np.full((6, 5, 2), -7, np.int16)
    fr = np.full((6, 5), 9, np.uint16)
    m23, m33 = np.eye(3)[:2].copy(), np.eye(3)
    p = lambda a: a.ctypes.data
    warp = lib.vp_warp_affine_u8(None, p(src), 5, 6, 1, p(m23), 0, 0, None, p(dst), 5, 6)
    assert warp == _vp.ERR_INVALID
    assert lib.vp_remap_u8(None, p(src), 5, 6, 1, p(mx), p(mx), 5, 6, 1, 0, None, p(dst)) == warp
    assert lib.vp_remap_f32_dev(None, p(src), 5, 5, 6, 1, p(mx), p(mx), 5, 6, 1, 0, None, p(dst)) == warp
    assert lib.vp_remap_fixed_dev(None, p(src), 5, 5, 6, 1, p(xy), p(fr), 5, 6, 1, 0, None, p(dst)) == warp
    assert lib.vp_convert_maps_dev(None, p(mx), p(mx), 5, 6, 0, p(xy), p(fr)) == warp
    assert lib.vp_warp_perspective_u8(None, p(src), 5, 6, 1, p(m33), 1, 0, None, p(dst), 5, 6) == warp
    assert lib.vp_warp_perspective_dev(None, p(src), 5, 5, 6, 1, p(m33), 1, 0, None, p(dst), 5, 6) == warp
    assert (dst == 77).all() and (xy == -7).all() and (fr == 9).all(), "a destination was written without a context"
