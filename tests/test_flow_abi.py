"""CPU suite for the surface of sparse optical flow (cv2.calcOpticalFlowPyrLK): the C entries are exported by libvp.so and declared in
include/vp.h with the prototypes vision/_vp.py binds; the units are built; the facade and vision.utils.feature have the names and cv2's
constants; every refusal comes from the arguments alone - VP_ERR_INVALID with its reason from the C entries, cv2_facade.error from the
facade, no device needed, nothing written."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from abi_header import _header_prototypes, header_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc")
NEW = ["vp_lk_flow_levels", "vp_lk_flow_dev", "vp_lk_flow_u8"]


def test_flow_symbols_are_exported_declared_and_bound_alike():
    from vision import _vp
    protos = _header_prototypes()
    lib = C.CDLL(_vp.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name) and name in protos and name in _vp._SIGS, name
        assert protos[name][0] == "int" and protos[name][1] == _vp._SIGS[name][1] and _vp._SIGS[name][0] is C.c_int, name
    assert [len(protos[n][1]) for n in NEW] == [5, 20, 16]
    built = open(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "build.py")).read()
    for src in ("vp_flow.hip", "vp_api_flow.hip"):
        assert f'"{src}"' in built, f"{src} is not among VP_SOURCES"
        assert os.path.exists(os.path.join(CSRC, src))
    assert os.path.exists(os.path.join(CSRC, "vp_flow_plan.h"))
    assert len(header_options()) == 11, "optical flow adds no option"
    kernel = open(os.path.join(CSRC, "vp_flow.hip")).read()
    assert '#include "vp_flow_plan.h"' in kernel and "__launch_bounds__(LK_LANES)" in kernel and "vp_lk_reflect" in kernel and "__dsqrt_rn" in kernel
    assert "cooperative" not in kernel and "grid.sync" not in kernel and "atomic" not in kernel


def test_level_rule_of_the_library_is_the_statements():
    import flow_restate as R
    from vision import _vp
    from vision.utils import feature
    lib = C.CDLL(_vp.LIB_PATH)
    lib.vp_lk_flow_levels.restype, lib.vp_lk_flow_levels.argtypes = _vp._SIGS["vp_lk_flow_levels"]
    assert lib.vp_lk_flow_levels(100, 90, 21, 21, 5) == 3 == feature.flow_level_count(100, 90, (21, 21), 5)
    for w, h, ww, wh, ml in ((100, 90, 21, 21, 1), (22, 22, 21, 21, 3), (21, 40, 21, 21, 3), (43, 43, 21, 21, 3), (42, 42, 21, 21, 3), (4096, 4096, 3, 3, 15),
                             (1920, 1080, 21, 21, 3), (160, 144, 63, 63, 3), (64, 4096, 63, 3, 15)):
        assert lib.vp_lk_flow_levels(w, h, ww, wh, ml) == R.level_count(w, h, ww, wh, ml) == feature.flow_level_count(w, h, (ww, wh), ml), (w, h, ww, wh, ml)
    assert lib.vp_lk_flow_levels(0, 5, 3, 3, 1) == 0 and lib.vp_lk_flow_levels(50, 50, 3, 3, -1) == 0


def test_facade_names_signatures_and_constants():
    from vision import cv2_facade as f
    from vision.utils import feature
    sig = lambda fn: [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(f.calcOpticalFlowPyrLK) == [("prevImg", E), ("nextImg", E), ("prevPts", E), ("nextPts", E), ("status", None), ("err", None), ("winSize", (21, 21)),
                                           ("maxLevel", 3), ("criteria", (3, 30, 0.01)), ("flags", 0), ("minEigThreshold", 1e-4)]
    assert (f.OPTFLOW_USE_INITIAL_FLOW, f.OPTFLOW_LK_GET_MIN_EIGENVALS) == (4, 8) == (feature.OPTFLOW_USE_INITIAL_FLOW, feature.OPTFLOW_LK_GET_MIN_EIGENVALS)
    assert sig(feature.track_points) == [("prev", E), ("next", E), ("pts", E), ("next_pts", None), ("win_size", (21, 21)), ("max_level", 3), ("max_count", 30),
                                         ("eps", 0.01), ("min_eig_threshold", 1e-4), ("min_eigenvals", False), ("back_check", None)]
    assert sig(feature.FlowPyramid.__init__)[1:] == [("mat", E), ("max_level", 3), ("win_size", (21, 21))]
    mod = f.install()
    for name in ("calcOpticalFlowPyrLK", "OPTFLOW_USE_INITIAL_FLOW", "OPTFLOW_LK_GET_MIN_EIGENVALS", "goodFeaturesToTrack", "pyrDown"):
        assert hasattr(mod, name), name
    for name in ("find_corners", "find_circles", "find_line_segments"):                 # the names that raise keep raising
        with pytest.raises(Exception):
            getattr(feature, name)(np.zeros((4, 4), np.uint8))


def test_facade_and_mirror_refuse_before_they_need_a_device():
    from vision import cv2_facade as f
    from vision.utils import feature
    grey, bgr = np.zeros((40, 50), np.uint8), np.zeros((40, 50, 3), np.uint8)
    pts = np.array([[[5, 5]], [[20, 20]]], np.float32)

    def refused(call, *words):
        with pytest.raises(f.error) as e:
            call()
        assert all(w in str(e.value) for w in words), str(e.value)

    lk = f.calcOpticalFlowPyrLK
    refused(lambda: lk(bgr, bgr, pts, None), "single-channel")
    refused(lambda: lk(grey.astype(np.float32), grey, pts, None), "uint8")
    refused(lambda: lk(grey, grey.astype(np.uint16), pts, None), "uint8")
    refused(lambda: lk(grey, np.zeros((40, 51), np.uint8), pts, None), "same size")
    refused(lambda: lk(grey, grey, pts, None, winSize=(2, 21)), "3 to 63")
    refused(lambda: lk(grey, grey, pts, None, winSize=(21, 64)), "3 to 63")
    refused(lambda: lk(grey, grey, pts, None, winSize=21), "two integers")
    refused(lambda: lk(grey, grey, pts, None, winSize=(50, 21)), "larger than the window")
    refused(lambda: lk(grey, grey, pts, None, winSize=(21, 40)), "larger than the window")
    refused(lambda: lk(grey, grey, pts, None, maxLevel=-1), "0 to 15")
    refused(lambda: lk(grey, grey, pts, None, maxLevel=16), "0 to 15")
    refused(lambda: lk(grey, grey, pts, None, flags=1), "unknown flag bits")
    refused(lambda: lk(grey, grey, pts, None, flags=4), "needs nextPts")
    refused(lambda: lk(grey, grey, pts, pts[:1], flags=4), "as many initial positions")
    refused(lambda: lk(grey, grey, pts, None, minEigThreshold=float("nan")), "finite")
    refused(lambda: lk(grey, grey, pts, None, criteria=(3, 30, float("inf"))), "finite")
    refused(lambda: lk(grey, grey, pts, None, criteria=None), "criteria")
    refused(lambda: lk(grey, grey, np.zeros((3, 3), np.float32), None), "pairs")
    refused(lambda: lk(np.zeros((40, 4097), np.uint8), np.zeros((40, 4097), np.uint8), pts, None), "4096")
    with pytest.raises(ValueError):
        feature.track_points(grey, grey, pts, back_check=-1)
    with pytest.raises(ValueError):
        feature.track_points(grey, grey, pts, back_check=float("nan"))


def test_c_refusals_come_from_the_arguments_alone_and_write_nothing():
    """Without a context an admitted call fails too (VP_ERR_INVALID, silently): what tells the refusals apart is the reason they leave in
    vp_last_error(NULL), which an admitted call does not touch."""
    from vision import _vp
    lib = C.CDLL(_vp.LIB_PATH)
    for name in NEW + ["vp_last_error"]:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _vp._SIGS[name]
    img = np.arange(60 * 80, dtype=np.uint8).reshape(60, 80)
    small = np.zeros((30, 40), np.uint8)
    pts = np.array([[5, 5], [20, 20], [70, 50]], np.float32)
    out = np.full((3, 4), 77, np.uint32)
    p = lambda a, off=0: None if a is None else a.ctypes.data + off
    why = lambda: lib.vp_last_error(None).decode()

    def put_marker():
        assert lib.vp_lk_flow_u8(None, None, None, 80, 60, None, None, 3, 21, 21, 3, 30, 0.01, 0, 1e-4, None) == _vp.ERR_INVALID
        return why()

    marker = put_marker()
    assert "pointer" in marker

    def admitted(rc):
        assert rc == _vp.ERR_INVALID and why() == marker, why()

    def refused(rc, words):
        assert rc == _vp.ERR_INVALID and words in why(), (words, why())
        assert put_marker() == marker

    def u8(a=img, b=img, w=80, h=60, pp=pts, ip=None, n=3, ww=21, wh=21, ml=3, mc=30, eps=0.01, fl=0, me=1e-4, o=out):
        return lib.vp_lk_flow_u8(None, p(a), p(b), w, h, p(pp), p(ip), n, ww, wh, ml, mc, eps, fl, me, p(o))

    def dev(levels=(img, small), nexts=None, strides=(80, 40), nl=None, w=80, h=60, pp=pts, ip=None, n=3, ww=21, wh=21, ml=3, mc=30, eps=0.01, fl=0, me=1e-4,
            od=out, oh=None, odoff=0, arrays=True):
        nexts = levels if nexts is None else nexts
        k = len(levels)
        pa = (C.c_void_p * k)(*[p(x) for x in levels])
        na = (C.c_void_p * k)(*[p(x) for x in nexts])
        sa = (C.c_size_t * k)(*strides)
        return lib.vp_lk_flow_dev(None, pa if arrays else None, sa, na, sa, k if nl is None else nl, w, h, p(pp), p(ip), n, ww, wh, ml, mc, eps, fl, me, p(od, odoff),
                                  p(oh))

    for call in (u8, dev):
        admitted(call())
        admitted(call(ww=3, wh=59))
        admitted(call(ww=63, wh=3))
        admitted(call(mc=-5, eps=-1.0))
        admitted(call(mc=100000, eps=1e9))
        admitted(call(ml=0))
        admitted(call(ml=15))
        admitted(call(fl=12, ip=pts))
        admitted(call(fl=8))
        admitted(call(n=1 << 20, **({"od": None, "oh": out} if call is dev else {})))    # (16 MiB of device result would overlap anything nearby)
        refused(call(w=0), "1 to 4096")
        refused(call(h=4097), "1 to 4096")
        refused(call(w=4097), "1 to 4096")
        refused(call(ww=2), "3 to 63")
        refused(call(wh=64), "3 to 63")
        refused(call(ww=63, wh=63), "larger than the window")
        refused(call(wh=60), "larger than the window")
        refused(call(n=0), "1 to 1048576 points")
        refused(call(n=(1 << 20) + 1), "1 to 1048576 points")
        refused(call(ml=-1), "0 to 15")
        refused(call(ml=16), "0 to 15")
        refused(call(fl=1), "unknown flag bits")
        refused(call(fl=4 | 16), "unknown flag bits")
        refused(call(me=float("nan")), "finite")
        refused(call(me=float("inf")), "finite")
        refused(call(eps=float("nan")), "finite")
        refused(call(eps=float("-inf")), "finite")
        refused(call(pp=None), "pointer")
        refused(call(fl=4), "pointer")                       # the initial flow is asked for and missing
    refused(u8(a=None), "pointer")
    refused(u8(b=None), "pointer")
    refused(u8(o=None), "pointer")
    refused(dev(arrays=False), "pointer")
    refused(dev(od=None, oh=None), "pointer")
    admitted(dev(od=None, oh=out))
    refused(dev(levels=(img, None)), "pointer")
    refused(dev(nexts=(None, small)), "pointer")
    admitted(dev(levels=(img, None), ml=0))                   # a level that is not used is not looked at
    admitted(dev(levels=(img, None), ww=41, wh=31))           # 40 x 30 is not above 41 x 31: one level
    refused(dev(nl=0), "1 to 16 pyramid levels")
    refused(dev(nl=17), "1 to 16 pyramid levels")
    refused(dev(strides=(79, 40)), "stride is below the row")
    refused(dev(strides=(80, 39)), "stride is below the row")
    admitted(dev(strides=(80, 39), ml=0))
    refused(dev(odoff=2), "aligned")
    refused(dev(od=img.view(np.uint32)), "overlaps")
    refused(dev(od=small.view(np.uint32)), "overlaps")
    admitted(dev(od=small.view(np.uint32), ml=0))
    assert (out == 77).all() and img[0, 1] == 1 and not small.any(), "a result was written without a context"
