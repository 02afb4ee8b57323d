"""CPU suite for the surface of cv2.moments / cv2.HuMoments: the six C entries are exported by libvp.so and declared in include/vp.h
with the prototypes vision/_vp.py binds; the two kernel units are built; the facade's dictionary has cv2's 24 keys in cv2's order and
HuMoments cv2's shape; the option is declared, documented and bound; every refusal of the raster and label entries comes from the
arguments alone - VP_ERR_INVALID with its reason, no context needed, nothing written."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import moments_restate as R
from abi_header import _header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vp_moments_u8", "vp_moments_dev", "vp_label_moments_i32", "vp_label_moments_dev", "vp_polygon_moments", "vp_moments_complete"]
CV2_KEYS = ["m00", "m10", "m01", "m20", "m11", "m02", "m30", "m21", "m12", "m03", "mu20", "mu11", "mu02", "mu30", "mu21", "mu12", "mu03",
            "nu20", "nu11", "nu02", "nu30", "nu21", "nu12", "nu03"]


def test_moments_symbols_are_exported_declared_and_bound_alike():
    from vision import _vp
    protos = _header_prototypes()
    lib = C.CDLL(_vp.LIB_PATH)
    for name in NEW:      # that each is bound as declared: test_abi.py::test_every_prototype_is_bound_as_declared
        assert hasattr(lib, name) and name in protos and name in _vp._SIGS, name
    assert len(protos["vp_moments_dev"][1]) == 8 and len(protos["vp_polygon_moments"][1]) == 4 and len(protos["vp_moments_complete"][1]) == 2
    built = open(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "build.py")).read()
    for src in ("vp_moments.hip", "vp_api_moments.hip"):
        assert f'"{src}"' in built, f"{src} is not among VP_SOURCES"
        assert os.path.exists(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc", src))


def test_plan_constants_and_the_option():
    from vision import _vp
    plan = open(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc", "vp_moments_plan.h")).read()
    num = lambda n: int(re.search(r"#define " + n + r" (\d+)", plan).group(1))
    assert num("MM_TB") % 64 == 0 and num("MM_SPAN") == 64 * num("MM_CHUNK") and num("MM_CHUNK") == 16 and num("MM_BIT_SPAN") == 64 * 64
    assert num("MM_ROWS") >= 1 and num("LM_ROWS") >= 1 and num("LM_SPAN") % 64 == 0
    assert num("LM_LDS_LABELS") * 80 <= 64 * 1024 < (num("LM_LDS_LABELS") + 64) * 80, "the LDS table is the largest that fits a block's 64 KiB (in steps of 64 labels)"
    assert 1 <= num("LM_HOT_LABELS") <= num("LM_LDS_LABELS"), "the rows a larger table keeps in LDS fit there"
    txt = open(os.path.join(ROOT, "include", "vp.h")).read()
    m = re.search(r"VP_OPT_LABEL_MOMENTS_LDS\s*=\s*(\d+)", txt)
    assert m and int(m.group(1)) == _vp.OPT_LABEL_MOMENTS_LDS == 11
    assert txt.count("VP_OPT_LABEL_MOMENTS_LDS") >= 3, "the option is documented with the others"


def test_facade_has_cv2s_names_keys_and_shapes():
    from vision import cv2_facade as f
    from vision.utils import feature
    assert list(inspect.signature(f.moments).parameters) == ["array", "binaryImage"] and inspect.signature(f.moments).parameters["binaryImage"].default is False
    assert list(inspect.signature(f.HuMoments).parameters)[0] == "m"
    assert list(feature.MOMENT_FIELDS) == CV2_KEYS == list(R.FIELDS)
    for c in (np.array([[[0, 0]], [[0, 5]], [[6, 5]], [[6, 0]]], np.int32), np.array([[0, 0], [0, 5], [6, 5]], np.float32), np.zeros((0, 1, 2), np.int32)):
        m = f.moments(c)
        assert type(m) is dict and list(m) == CV2_KEYS and all(type(v) is float for v in m.values())
        assert R.as_bytes(list(m.values())) == R.as_bytes(R.complete(R.contour_moments(c)))
        hu = f.HuMoments(m)
        assert type(hu) is np.ndarray and hu.dtype == np.float64 and hu.shape == (7, 1)
        assert hu.tobytes() == R.as_bytes(R.hu(R.complete(R.contour_moments(c))))
    sig = lambda fn: list(inspect.signature(fn).parameters)
    assert sig(feature.image_moments) == ["mat", "binary"] and sig(feature.component_moments) == ["labels", "nlabels"]
    assert sig(feature.moments_dict) == ["row"] and sig(feature.hu_moments) == sig(feature.orientation) == ["m"] and sig(feature.contour_moments) == ["contour"]
    assert f.install() is not None and hasattr(f.install(), "moments") and hasattr(f.install(), "HuMoments")


def test_facade_refuses_what_is_outside_the_path_before_it_needs_a_device():
    from vision import cv2_facade as f
    for bad in (np.zeros((4, 2), np.int64), np.zeros((4, 2), np.float64), np.zeros((1, 4, 2), np.int32), np.zeros((4, 3), np.int32), np.zeros((4, 5, 3), np.uint8),
                np.zeros((4, 5), np.uint16), np.zeros((0, 5), np.uint8), [[0, 0], [1, 1], [2, 0]], None):
        with pytest.raises(f.error):
            f.moments(bad)
    for bad in ({}, {"m00": 1.0}, None, np.zeros(24)):
        with pytest.raises(f.error):
            f.HuMoments(bad)


def _bound_ok(w, h, vmax):
    """the admission of the issue: vmax * h * sum_{x < w} x^3, and the transpose, below 2^63"""
    sx, sy = (w * (w - 1) // 2) ** 2, (h * (h - 1) // 2) ** 2
    return vmax * h * sx < 2 ** 63 and vmax * w * sy < 2 ** 63


def _largest_width(h, vmax):
    lo, hi = 1, 1 << 20
    while lo + 1 < hi:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if _bound_ok(mid, h, vmax) else (lo, mid)
    return lo


def test_refusals_come_from_the_arguments_alone_and_write_nothing():
    """Without a context an admitted call fails too (VP_ERR_INVALID, silently): what tells the refusals apart is the reason they
    leave in vp_last_error(NULL), which an admitted call does not touch."""
    from vision import _vp
    lib = C.CDLL(_vp.LIB_PATH)
    for name in NEW + ["vp_last_error"]:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _vp._SIGS[name]
    src = np.arange(35, dtype=np.uint8).reshape(5, 7)
    lab = np.zeros((5, 7), np.int32)
    out = np.full(64, 77, np.uint64)
    p = lambda a: a.ctypes.data
    why = lambda: lib.vp_last_error(None).decode()

    def admitted(rc):
        """no new reason: the marker is still there"""
        assert rc == _vp.ERR_INVALID and why() == marker, why()

    def refused(rc, words):
        assert rc == _vp.ERR_INVALID and words in why(), (words, why())
        assert lib.vp_moments_u8(None, None, 7, 7, 5, 0, p(out)) == _vp.ERR_INVALID and why() == marker      # put the marker back

    assert lib.vp_moments_u8(None, None, 7, 7, 5, 0, p(out)) == _vp.ERR_INVALID
    marker = why()
    assert "pointer" in marker
    admitted(lib.vp_moments_u8(None, p(src), 7, 7, 5, 0, p(out)))
    admitted(lib.vp_moments_dev(None, p(src), 9, 7, 5, 1, None, p(out)))
    admitted(lib.vp_label_moments_i32(None, p(lab), 28, 7, 5, 3, p(out)))
    admitted(lib.vp_label_moments_dev(None, p(lab), 32, 7, 5, 5000, p(out)))
    for host in (True, False):
        call = (lambda *a: lib.vp_moments_u8(None, p(src), *a, p(out))) if host else (lambda *a: lib.vp_moments_dev(None, p(src), *a, None, p(out)))
        refused(call(7, 0, 5, 0), "at least 1")
        refused(call(7, 7, 0, 0), "at least 1")
        refused(call(7, 7, -2, 1), "at least 1")
        refused(call(7, 7, 65536, 1), "65535")
        admitted(call(7, 1, 65535, 1))
        refused(call(2, 2, 65535, 0), "2^63")
        refused(call(6, 7, 5, 0), "stride")
        for vmax, binary in ((255, 0), (1, 1)):
            for h in (1, 2, 1080):
                w = _largest_width(h, vmax)
                assert _bound_ok(w, h, vmax) and not _bound_ok(w + 1, h, vmax)
                admitted(call(w, w, h, binary))
                refused(call(w + 1, w + 1, h, binary), "2^63")
            tall = max(hh for hh in (65535, 30000, 19000, 10000) if _bound_ok(2, hh, vmax))     # the transpose: m03 of a tall image
            admitted(call(2, 2, tall, binary))
        refused(call(40000, 40000, 65535, 0), "2^63")
    assert _bound_ok(1920, 1080, 255) and _largest_width(1080, 255) > 1920, "all-255 1080p is admitted"
    refused(lib.vp_moments_dev(None, None, 7, 7, 5, 1, None, p(out)), "pointer")
    refused(lib.vp_moments_dev(None, p(src), 7, 7, 5, 0, p(out), p(out)), "binary")
    for fn in (lib.vp_label_moments_i32, lib.vp_label_moments_dev):
        refused(fn(None, p(lab), 28, 7, 5, 0, p(out)), "nlabels")
        refused(fn(None, p(lab), 28, 7, 5, -3, p(out)), "nlabels")
        refused(fn(None, p(lab), 28, 0, 5, 2, p(out)), "at least 1")
        refused(fn(None, p(lab), 28, 7, 65536, 2, p(out)), "65535")
        refused(fn(None, p(lab), 24, 7, 5, 2, p(out)), "stride")
        refused(fn(None, p(lab), 30, 7, 5, 2, p(out)), "aligned")
        refused(fn(None, None, 28, 7, 5, 2, p(out)), "pointer")
        w = _largest_width(1, 1)
        admitted(fn(None, p(lab), 4 * w, w, 1, 2, p(out)))
        refused(fn(None, p(lab), 4 * (w + 1), w + 1, 1, 2, p(out)), "2^63")
    assert (out == 77).all(), "a result was written without a context"
