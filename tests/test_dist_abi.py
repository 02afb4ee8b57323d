"""CPU suite for the surface of cv2.distanceTransform / cv2.minMaxLoc: the four C entries are exported by libvp.so and declared in
include/vp.h with the prototypes vision/_vp.py binds; the two units are built; the plan's constants are readable and its LDS
arithmetic stays within 64 KiB; the facade has cv2's signatures and defaults; every refusal comes from the arguments alone -
VP_ERR_INVALID with its reason from the C entries, cv2_facade.error from the facade, no device needed, nothing written."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from abi_header import _header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc")
NEW = ["vp_distance_transform_u8", "vp_distance_transform_dev", "vp_min_max_loc_u8", "vp_min_max_loc_dev"]


def test_dist_symbols_are_exported_declared_and_bound_alike():
    from vision import _vp
    protos = _header_prototypes()
    lib = C.CDLL(_vp.LIB_PATH)
    for name in NEW:      # that each is bound as declared: test_abi.py::test_every_prototype_is_bound_as_declared
        assert hasattr(lib, name) and name in protos and name in _vp._SIGS, name
    assert [len(protos[n][1]) for n in NEW] == [7, 10, 11, 12]
    built = open(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "build.py")).read()
    for src in ("vp_dist.hip", "vp_api_dist.hip"):
        assert f'"{src}"' in built, f"{src} is not among VP_SOURCES"
        assert os.path.exists(os.path.join(CSRC, src))
    assert (_vp.DIST_L1, _vp.DIST_L2, _vp.DIST_C) == (1, 2, 3)
    header = open(os.path.join(ROOT, "include", "vp.h")).read()
    assert "VP_DIST_L1 = 1, VP_DIST_L2 = 2, VP_DIST_C = 3" in header


def test_plan_constants_are_readable_and_prove_the_bounds():
    plan = open(os.path.join(CSRC, "vp_dist_plan.h")).read()
    num = lambda n: int(re.search(r"#define " + n + r" (\d+)", plan).group(1))
    side, none, lds, px = num("DT_MAX_SIDE"), num("DT_NONE"), num("DT_LDS_BYTES"), num("DT_PX")
    scols, srows, wcols, wrows = num("DT_STRIP_COLS"), num("DT_STRIP_ROWS"), num("DT_WIDE_COLS"), num("DT_WIDE_ROWS")
    assert side == 4096 and lds == 64 * 1024 and px == 4
    assert "#define DT_STAGED_MAX_H (DT_LDS_BYTES / (DT_STRIP_COLS * 2))" in plan and "#define DT_SWITCH_H (DT_STAGED_MAX_H + 1)" in plan
    staged_max = lds // (scols * 2)
    assert staged_max * scols * 2 <= 64 * 1024, "the staged strip of the tallest image it takes is above 64 KiB of LDS"
    assert "static_assert(DT_STAGED_MAX_H * DT_STRIP_COLS * 2 <= DT_LDS_BYTES" in plan
    assert staged_max + 1 <= side, "the direct form is never taken: the switch test of the GPU suite would test nothing"
    for cols, rows in ((scols, srows), (wcols, wrows)):
        assert cols % px == 0 and 64 % cols == 0 and 256 % (cols // px) == 0 and rows % (256 // (cols // px)) == 0
    # every true distance is below the sentinel's cost, every cost fits int32, squares are exact in float32, the raster index fits the key
    assert 2 * (side - 1) ** 2 < none * none and none * none + (side - 1) ** 2 < 2 ** 31 and 2 * (side - 1) < min(none, 8192)
    assert (side - 1) ** 2 < 2 ** 24 and side * side <= 2 ** 24 and none < 2 ** 16
    kernels = open(os.path.join(CSRC, "vp_dist.hip")).read()
    assert "vp_dist_lds_bytes(h)" in kernels and "vp_mml_key" in kernels and "vp_corner_key" in plan


def test_facade_signatures_and_defaults_are_cv2s():
    from vision import cv2_facade as f
    from vision.utils import feature
    sig = lambda fn: [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(f.distanceTransform) == [("src", E), ("distanceType", E), ("maskSize", E), ("dst", None), ("dstType", 5)]
    assert sig(f.minMaxLoc) == [("src", E), ("mask", None)]
    assert sig(feature.distance_transform) == [("mat", E), ("metric", 2), ("dst_type", np.float32)]
    assert sig(feature.min_max_loc) == [("mat", E), ("mask", None)]
    assert sig(feature.largest_inscribed_circle) == [("mask", E)]
    want = dict(DIST_USER=-1, DIST_L1=1, DIST_L2=2, DIST_C=3, DIST_L12=4, DIST_FAIR=5, DIST_WELSCH=6, DIST_HUBER=7, DIST_MASK_3=3, DIST_MASK_5=5,
                DIST_MASK_PRECISE=0)
    assert {k: getattr(f, k) for k in want} == want
    m = f.install()
    assert all(hasattr(m, n) for n in ("distanceTransform", "minMaxLoc"))
    assert "nearest zero pixel's centre" in feature.largest_inscribed_circle.__doc__ or "centre of the\n    nearest zero pixel" in feature.largest_inscribed_circle.__doc__


def test_facade_refuses_what_is_outside_the_contract_before_it_needs_a_device():
    from vision import cv2_facade as f
    img = np.zeros((9, 11), np.uint8)
    for size in (f.DIST_MASK_3, f.DIST_MASK_5):
        with pytest.raises(f.error, match="DIST_MASK_PRECISE"):
            f.distanceTransform(img, f.DIST_L2, size)
    bad_images = (np.zeros((9, 11), np.uint16), np.zeros((9, 11), np.float32), np.zeros((9, 11, 3), np.uint8), np.zeros((0, 11), np.uint8), None,
                  np.zeros((3, 4097), np.uint8), np.zeros((4097, 3), np.uint8))
    for bad in bad_images:
        with pytest.raises(f.error):
            f.distanceTransform(bad, f.DIST_L2, f.DIST_MASK_PRECISE)
    for metric in (f.DIST_USER, f.DIST_L12, f.DIST_FAIR, f.DIST_WELSCH, f.DIST_HUBER, 0, 8):
        with pytest.raises(f.error):
            f.distanceTransform(img, metric, f.DIST_MASK_3)
    for call in (lambda: f.distanceTransform(img, f.DIST_L1, 4), lambda: f.distanceTransform(img, f.DIST_C, 7),
                 lambda: f.distanceTransform(img, f.DIST_L2, f.DIST_MASK_PRECISE, None, f.CV_8U), lambda: f.distanceTransform(img, f.DIST_C, 3, None, f.CV_8U),
                 lambda: f.distanceTransform(img, f.DIST_L1, 3, None, f.CV_16S), lambda: f.distanceTransform(img, f.DIST_L1, 3, None, f.CV_64F)):
        with pytest.raises(f.error):
            call()
    assert not hasattr(f, "distanceTransformWithLabels")
    for bad in (np.zeros((9, 11), np.uint16), np.zeros((9, 11), np.float64), np.zeros((9, 11, 3), np.uint8), np.zeros((9, 11, 2), np.float32),
                np.zeros((0, 11), np.uint8), None, np.zeros((3, 4097), np.float32)):
        with pytest.raises(f.error):
            f.minMaxLoc(bad)
    for mask in (np.zeros((9, 10), np.uint8), np.zeros((9, 11), np.float32), np.zeros((9, 11, 3), np.uint8)):
        with pytest.raises(f.error):
            f.minMaxLoc(img, mask)
        with pytest.raises(f.error):
            f.minMaxLoc(img.astype(np.float32), mask)


def test_c_refusals_come_from_the_arguments_alone_and_write_nothing():
    """Without a context an admitted call fails too (VP_ERR_INVALID, silently): what tells the refusals apart is the reason they leave in
    vp_last_error(NULL), which an admitted call does not touch."""
    from vision import _vp
    lib = C.CDLL(_vp.LIB_PATH)
    for name in NEW + ["vp_last_error"]:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _vp._SIGS[name]
    src = np.arange(35, dtype=np.uint8).reshape(5, 7)
    fsrc = np.arange(35, dtype=np.float32).reshape(5, 7)
    mask = np.full((8, 8), 255, np.uint8)
    dst = np.full((5, 8), 77.0, np.float32)
    out = np.full(4, 77.0, np.float64)
    p = lambda a: a.ctypes.data
    why = lambda: lib.vp_last_error(None).decode()
    L1, L2, CH, U8, F32 = 1, 2, 3, 0, 5

    def put_marker():
        assert lib.vp_distance_transform_u8(None, None, 7, 5, L2, F32, p(dst)) == _vp.ERR_INVALID
        return why()

    marker = put_marker()
    assert "pointer" in marker

    def admitted(rc):
        assert rc == _vp.ERR_INVALID and why() == marker, why()

    def refused(rc, words):
        assert rc == _vp.ERR_INVALID and words in why(), (words, why())
        assert put_marker() == marker

    host = lambda w=7, h=5, metric=L2, depth=F32, s=src, d=dst: lib.vp_distance_transform_u8(None, None if s is None else p(s), w, h, metric, depth,
                                                                                              None if d is None else p(d))
    for metric in (L1, L2, CH):
        admitted(host(metric=metric))
    admitted(host(metric=L1, depth=U8))
    admitted(host(w=4096, h=4096))
    refused(host(w=0), "at least 1")
    refused(host(h=-1), "at least 1")
    refused(host(w=4097), "4096")
    refused(host(h=4097), "4096")
    for metric in (0, 4, 5, 6, 7, -1):
        refused(host(metric=metric), "metric")
    refused(host(metric=L2, depth=U8), "only with DIST_L1")
    refused(host(metric=CH, depth=U8), "only with DIST_L1")
    for depth in (3, 4, 6, -1):
        refused(host(depth=depth), "CV_8U or CV_32F")
    refused(host(d=None), "pointer")

    def dev(stride=7, w=7, h=5, bits=None, metric=L2, depth=F32, s=src, d=dst, dstride=32, doff=0):
        return lib.vp_distance_transform_dev(None, None if s is None else p(s), stride, w, h, bits, metric, depth, None if d is None else p(d) + doff, dstride)

    admitted(dev())
    admitted(dev(stride=9, dstride=28))
    admitted(dev(bits=p(mask)))
    admitted(dev(metric=L1, depth=U8, dstride=7))
    admitted(dev(metric=L1, depth=U8, dstride=9))
    refused(dev(w=0), "at least 1")
    refused(dev(h=4097), "4096")
    refused(dev(stride=6), "stride is below the row")
    refused(dev(dstride=27), "result's stride is below the row")
    refused(dev(dstride=30), "multiple of the element size")
    refused(dev(metric=L1, depth=U8, dstride=6), "result's stride is below the row")
    refused(dev(metric=9), "metric")
    refused(dev(metric=CH, depth=U8, dstride=7), "only with DIST_L1")
    refused(dev(depth=6), "CV_8U or CV_32F")
    refused(dev(s=None, bits=p(mask)), "bit plane without its source")
    refused(dev(s=None), "pointer")
    refused(dev(d=None), "pointer")
    refused(dev(bits=p(mask) + 4), "8-byte")
    refused(dev(doff=2), "aligned")
    refused(lib.vp_distance_transform_dev(None, p(dst), 7, 7, 5, None, L2, F32, p(dst), 32), "overlaps")

    def mhost(stride=7, w=7, h=5, depth=U8, s=src, m=None, ms=0, mw=0, mh=0, o=out):
        return lib.vp_min_max_loc_u8(None, None if s is None else p(s), stride, w, h, depth, None if m is None else p(m), ms, mw, mh, None if o is None else p(o))

    def mdev(stride=7, w=7, h=5, depth=U8, s=src, m=None, ms=0, mw=0, mh=0, o=out, bits=None):
        return lib.vp_min_max_loc_dev(None, None if s is None else p(s), stride, w, h, depth, None if m is None else p(m), ms, mw, mh, bits,
                                      None if o is None else p(o))

    for call in (mhost, mdev):
        admitted(call())
        admitted(call(stride=9))
        admitted(call(depth=F32, s=fsrc, stride=28))
        admitted(call(depth=F32, s=fsrc, stride=32))
        admitted(call(m=mask, ms=8, mw=7, mh=5))
        refused(call(w=0), "at least 1")
        refused(call(w=4097, stride=4097), "4096")
        refused(call(h=4097), "4096")
        refused(call(stride=6), "stride is below the row")
        refused(call(depth=F32, s=fsrc, stride=24), "stride is below the row")
        refused(call(depth=F32, s=fsrc, stride=30), "multiple of the element size")
        for depth in (3, 4, 6, -1):
            refused(call(depth=depth), "8U or 32F")
        refused(call(m=mask, ms=8, mw=6, mh=5), "size of the image")
        refused(call(m=mask, ms=8, mw=7, mh=6), "size of the image")
        refused(call(m=mask, ms=6, mw=7, mh=5), "mask's stride")
        refused(call(s=None), "pointer")
        refused(call(o=None), "pointer")
    admitted(mdev(bits=p(mask), mw=7, mh=5))
    refused(mdev(bits=p(mask) + 4, mw=7, mh=5), "8-byte")
    refused(mdev(bits=p(mask), mw=7, mh=4), "size of the image")
    refused(lib.vp_min_max_loc_dev(None, p(fsrc) + 2, 28, 7, 5, F32, None, 0, 0, 0, None, p(out)), "4-byte")
    assert (dst == 77.0).all() and (out == 77.0).all(), "a result was written without a context"
