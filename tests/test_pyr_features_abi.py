"""CPU suite for the surface of the features over a scale pyramid: the three entries are exported by
libvp.so and declared in include/vp.h with the prototypes vision/_vp.py binds; vp_pyr_features_plan gives the statement's level sizes
and quotas; every refusal comes from the arguments alone - VP_ERR_INVALID with its reason, no device needed, nothing written;
PyramidSIFT and pyramid_features have the stated signatures, and SIFT keeps its own."""
import ctypes as C
import inspect

import numpy as np
import pytest

from abi_header import _header_prototypes
import features_cases as K
import pyr_features_restate as P

NEW = ["vp_pyr_features_plan", "vp_pyr_features_u8", "vp_pyr_features_dev"]


def library():
    return K.library(("vp_pyr_features_", "vp_describe_"))


def test_pyramid_symbols_are_exported_declared_and_bound_alike():
    from vision import _vp
    protos = _header_prototypes()
    lib = C.CDLL(_vp.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name) and name in protos and name in _vp._SIGS, name
        assert protos[name][1] == list(_vp._SIGS[name][1]) and protos[name][0] == "int", name
    assert len(protos["vp_pyr_features_plan"][1]) == 7 and len(protos["vp_pyr_features_u8"][1]) == len(protos["vp_pyr_features_dev"][1]) == 15


def test_plan_gives_the_statements_sizes_and_quotas():
    lib = library()
    n, wh, quota = C.c_int(-7), np.full((8, 2), -7, np.int32), np.full(8, -7, np.int32)
    for side in range(25, 201):
        for other in (side, 31, 200):
            for levels in range(1, 9):
                for budget in (0, 1, 100, 2000):
                    wh[:], quota[:] = -7, -7
                    assert lib.vp_pyr_features_plan(side, other, levels, budget, C.addressof(n), wh.ctypes.data, quota.ctypes.data) == 0
                    sizes = P.level_sizes(side, other, levels)
                    assert n.value == len(sizes) and wh[:n.value].tolist() == [list(s) for s in sizes], (side, other, levels)
                    assert quota[:n.value].tolist() == P.quotas(sizes, budget) and (wh[n.value:] == -7).all() and (quota[n.value:] == -7).all()
    assert lib.vp_pyr_features_plan(1920, 1080, 8, 1 << 20, C.addressof(n), wh.ctypes.data, quota.ctypes.data) == 0
    sizes = P.level_sizes(1920, 1080, 8)
    assert n.value == 8 and wh.tolist() == [list(s) for s in sizes] and quota.tolist() == P.quotas(sizes, 1 << 20) and int(quota.sum()) == 1 << 20
    why = lambda: lib.vp_last_error(None).decode()
    n.value = -7
    for args, words in (((100, 100, 0, 10), "levels"), ((100, 100, 9, 10), "levels"), ((100, 100, 8, -1), "negative"), ((100, 100, 8, (1 << 20) + 1), "1048576"),
                        ((0, 100, 8, 10), "at least 1"), ((65536, 100, 8, 10), "65535"), ((8193, 8192, 8, 10), "2^26")):
        assert lib.vp_pyr_features_plan(*args, C.addressof(n), wh.ctypes.data, quota.ctypes.data) != 0 and words in why(), (args, why())
    assert lib.vp_pyr_features_plan(100, 100, 8, 10, None, wh.ctypes.data, quota.ctypes.data) != 0 and "pointer" in why()
    assert lib.vp_pyr_features_plan(100, 100, 8, 10, C.addressof(n), None, quota.ctypes.data) != 0 and "pointer" in why()
    assert n.value == -7


def test_c_refusals_come_from_the_arguments_alone_and_write_nothing():
    """Without a context an admitted call fails too (VP_ERR_INVALID, silently): what tells the refusals apart is the reason they leave in
    vp_last_error(NULL), which an admitted call does not touch (as tests/test_features_abi.py does it)."""
    from vision import _vp
    lib = library()
    src = np.arange(40 * 40, dtype=np.uint8).reshape(40, 40)
    xy0, lxy, val = np.full((16, 2), 77, np.float32), np.full((16, 3), 77, np.int32), np.full(16, 77, np.int32)
    bins, desc, n = np.full(16, 77, np.uint8), np.full((16, 32), 77, np.uint8), C.c_int(77)
    p = lambda a: None if a is None else a.ctypes.data
    why = lambda: lib.vp_last_error(None).decode()

    def put_marker():
        assert lib.vp_describe_pattern(None) == _vp.ERR_INVALID
        return why()

    marker = put_marker()

    def admitted(rc):
        assert rc == _vp.ERR_INVALID and why() == marker, why()

    def refused(rc, words):
        assert rc == _vp.ERR_INVALID and words in why(), (words, why())
        assert put_marker() == marker

    for fn in (lib.vp_pyr_features_u8, lib.vp_pyr_features_dev):
        call = lambda s=src, stride=40, w=40, h=40, levels=8, thr=20, cap=16, a=xy0, b=lxy, c=val, d=bins, e=desc, dev=None, cnt=n: fn(
            None, p(s), stride, w, h, levels, thr, cap, p(a), p(b), p(c), p(d), p(e), dev, None if cnt is None else C.addressof(cnt))
        admitted(call())
        admitted(call(w=30, h=30))                                  # no level: not an error
        admitted(call(w=1, h=1))
        admitted(call(levels=1, thr=0))
        admitted(call(thr=255, stride=48, w=33))
        admitted(call(cap=0, a=None, b=None, c=None, d=None, e=None))
        admitted(call(cap=1 << 20))
        admitted(call(dev=4096))
        refused(call(levels=0), "levels must be 1 to 8")
        refused(call(levels=9), "levels must be 1 to 8")
        refused(call(thr=-1), "0 to 255")
        refused(call(thr=256), "0 to 255")
        refused(call(cap=-1), "negative")
        refused(call(cap=(1 << 20) + 1), "1048576")
        refused(call(stride=39), "stride")
        refused(call(w=0), "at least 1")
        refused(call(h=-3), "at least 1")
        refused(call(w=65536, stride=65536), "65535")
        refused(call(h=65536), "65535")
        refused(call(w=8193, stride=8193, h=8192), "2^26")
        refused(call(w=65535, stride=65535, h=65535), "2^26")
        refused(call(dev=4100), "aligned")
        for missing in ("s", "a", "b", "c", "d", "e", "cnt"):
            refused(call(**{missing: None}), "pointer")
    assert (xy0 == 77).all() and (lxy == 77).all() and (val == 77).all() and (bins == 77).all() and (desc == 77).all() and n.value == 77, "written without a context"


def test_python_names_and_signatures():
    from vision import cv2_facade as f
    from vision.utils import feature, sift
    sig = lambda fn: [(q.name, q.default) for q in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(feature.pyramid_features) == [("mat", E), ("threshold", 20), ("max_points", 2000), ("levels", 8), ("device_descriptors", False)]
    assert sig(sift.PyramidSIFT.__init__)[1:] == [("checks", 50), ("levels", 8)] and issubclass(sift.PyramidSIFT, sift.SIFT)
    assert sift.PyramidSIFT.match is sift.SIFT.match and sift.PyramidSIFT._detect is not sift.SIFT._detect
    assert sift.PyramidSIFT().levels == 8 and sift.PyramidSIFT(levels=3).levels == 3 and sift.PyramidSIFT().sources == {}
    # what tests/test_features_abi.py pins for SIFT stays
    assert sig(sift.SIFT.__init__)[1:] == [("checks", 50)] and sig(sift.SIFT.match)[1:] == [("img", E), ("min_match", 10), ("ratio", 0.7), ("draw", False)]
    doc = sift.SIFT.__doc__ + sift.__doc__
    assert "single-scale binary features" in doc and "not scale-invariant SIFT" in doc and "PyramidSIFT" in sift.__doc__
    assert sig(feature.match_descriptors) == [("query", E), ("train", E), ("k", 2), ("cross_check", False)]
    assert not hasattr(f, "ORB_create")
    assert feature.pyramid_level_sizes(1920, 1080, 8) == P.level_sizes(1920, 1080, 8) and feature.pyramid_level_sizes(36, 37) == [(36, 37)]
    img = np.zeros((40, 40), np.uint8)
    for call in (lambda: feature.pyramid_features(img, -1), lambda: feature.pyramid_features(img, 256), lambda: feature.pyramid_features(img, 20, -1),
                 lambda: feature.pyramid_features(img, 20, (1 << 20) + 1), lambda: feature.pyramid_features(img, 20, 10, 0), lambda: feature.pyramid_features(img, 20, 10, 9),
                 lambda: feature.pyramid_features(np.zeros((40, 40, 3), np.uint8)), lambda: feature.pyramid_features(img.astype(np.float32))):
        with pytest.raises((ValueError, TypeError)):
            call()
