"""CPU suite for the surface of cv2.matchTemplate: the two C entries are exported by libvp.so and declared in include/vp.h with the
prototypes vision/_vp.py binds; the three units are built; the plan's constants are readable and prove the bounds - N cn <= 65536
keeps every sum in uint32 and a block's LDS under the limit; the facade has cv2's signature and defaults; every refusal comes from the
arguments alone - VP_ERR_INVALID with its reason from the C entries, cv2_facade.error from the facade, no device needed, nothing
written."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from abi_header import _header_prototypes, header_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc")
NEW = ["vp_match_template_u8", "vp_match_template_dev"]


def test_match_symbols_are_exported_declared_and_bound_alike():
    from vision import _vp
    protos = _header_prototypes()
    lib = C.CDLL(_vp.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name) and name in protos and name in _vp._SIGS, name
        assert protos[name][0] == "int" and protos[name][1] == _vp._SIGS[name][1] and _vp._SIGS[name][0] is C.c_int, name
    assert [len(protos[n][1]) for n in NEW] == [10, 13]
    built = open(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "build.py")).read()
    for src in ("vp_match.hip", "vp_api_match.hip"):
        assert f'"{src}"' in built, f"{src} is not among VP_SOURCES"
        assert os.path.exists(os.path.join(CSRC, src))
    assert os.path.exists(os.path.join(CSRC, "vp_match_plan.h"))
    assert (_vp.TM_SQDIFF, _vp.TM_SQDIFF_NORMED, _vp.TM_CCORR, _vp.TM_CCORR_NORMED, _vp.TM_CCOEFF, _vp.TM_CCOEFF_NORMED) == (0, 1, 2, 3, 4, 5)
    header = open(os.path.join(ROOT, "include", "vp.h")).read()
    assert "VP_TM_SQDIFF = 0, VP_TM_SQDIFF_NORMED = 1, VP_TM_CCORR = 2, VP_TM_CCORR_NORMED = 3, VP_TM_CCOEFF = 4, VP_TM_CCOEFF_NORMED = 5" in header
    assert len(header_options()) == 11, "template matching adds no option"


def test_plan_constants_are_readable_and_prove_the_bounds():
    plan = open(os.path.join(CSRC, "vp_match_plan.h")).read()
    num = lambda n: int(re.search(r"#define " + n + r" (\d+)", plan).group(1))
    side, maxcn, elems, lds = num("MT_MAX_SIDE"), num("MT_MAX_CN"), num("MT_MAX_ELEMS"), num("MT_LDS_BYTES")
    rx, ry, lx, ly, threads = num("MT_RX"), num("MT_RY"), num("MT_LANES_X"), num("MT_LANES_Y"), num("MT_THREADS")
    tile_w, tile_h, rows, words, slack = num("MT_TILE_W"), num("MT_TILE_H"), num("MT_CHUNK_ROWS"), num("MT_CHUNK_WORDS"), num("MT_PATCH_SLACK")
    assert (side, maxcn, elems, lds) == (4096, 4, 65536, 64 * 1024)
    assert threads == lx * ly == 256 and tile_w == lx * rx and tile_h == ly * ry and rx == 4 and words % 4 == 0
    # N cn <= 65536 bytes of at most 255: C, S2 and T2 fit uint32 but not int32, N times a sum stays below 2^48 (exact in double)
    top = 255 * 255 * elems
    assert 2 ** 31 < top < 2 ** 32 and top * elems < 2 ** 48 and 255 * elems < 2 ** 24
    assert "static_assert(255ull * 255ull * MT_MAX_ELEMS < (1ull << 32)" in plan and "static_assert(255ull * 255ull * MT_MAX_ELEMS * MT_MAX_ELEMS < (1ull << 48)" in plan
    # LDS of the largest block, as vp_match_make_plan sizes it: a full chunk under a full tile of 4-channel results
    patch = (tile_h + rows - 1) * (lx * maxcn + words + slack)
    chunk = (rows + 2 * (ry - 1)) * words
    assert ((patch + 3) // 4 * 4 + chunk) * 4 <= lds
    assert "P->lds_bytes = ((size_t)P->templ_off + (size_t)(P->chunk_rows + 2 * (MT_RY - 1)) * P->chunk_words) * 4;" in plan
    assert "P->patch_pitch = MT_LANES_X * cn + P->chunk_words + MT_PATCH_SLACK;" in plan and "P->patch_rows = MT_TILE_H + P->chunk_rows - 1;" in plan
    # the chunked path exists within the size limit both ways: more rows than a chunk, more words than a chunk
    assert rows + 1 <= side and (rows + 1) * 1 <= elems and 4 * words + 1 <= side
    kernels = open(os.path.join(CSRC, "vp_match.hip")).read()
    assert "__builtin_amdgcn_udot4" in kernels and "__builtin_amdgcn_alignbyte" in kernels and "__ddiv_rn" in kernels and "__dsqrt_rn" in kernels
    assert "u32 acc[MT_RY][MT_RX];" in kernels, "the accumulators must be unsigned"
    assert "P.lds_bytes" in kernels and '#include "vp_match_plan.h"' in kernels


def test_facade_signature_and_defaults_are_cv2s():
    from vision import cv2_facade as f
    from vision.utils import feature
    sig = lambda fn: [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(f.matchTemplate) == [("image", E), ("templ", E), ("method", E), ("result", None), ("mask", None)]
    assert sig(feature.match_template) == [("mat", E), ("templ", E), ("method", 5)]
    assert sig(feature.best_match) == [("mat", E), ("templ", E), ("method", 5)]
    want = dict(TM_SQDIFF=0, TM_SQDIFF_NORMED=1, TM_CCORR=2, TM_CCORR_NORMED=3, TM_CCOEFF=4, TM_CCOEFF_NORMED=5)
    assert {k: getattr(f, k) for k in want} == want == {k: getattr(feature, k) for k in want}
    assert hasattr(f.install(), "matchTemplate")


def test_facade_refuses_what_is_outside_the_contract_before_it_needs_a_device():
    from vision import cv2_facade as f
    from vision.utils import feature
    img, templ = np.zeros((9, 11), np.uint8), np.zeros((3, 4), np.uint8)
    bgr, tbgr = np.zeros((9, 11, 3), np.uint8), np.zeros((3, 4, 3), np.uint8)
    with pytest.raises(f.error, match="mask"):
        f.matchTemplate(img, templ, f.TM_CCORR, None, np.ones((3, 4), np.uint8))
    for a, b in ((img, np.zeros((10, 4), np.uint8)), (img, np.zeros((3, 12), np.uint8)), (templ, img)):
        with pytest.raises(f.error, match="larger than the image"):
            f.matchTemplate(a, b, f.TM_CCORR)
    for a, b in ((bgr, templ), (img, tbgr), (bgr, np.zeros((3, 4, 4), np.uint8)), (np.zeros((9, 11, 1), np.uint8), np.zeros((3, 4, 2), np.uint8))):
        with pytest.raises(f.error, match="channels"):
            f.matchTemplate(a, b, f.TM_CCORR)
    for bad in (img.astype(np.float32), img.astype(np.uint16), img.astype(np.int8), None, np.zeros((0, 11), np.uint8), np.zeros((9, 11, 5), np.uint8),
                np.zeros((2, 3, 4, 5), np.uint8)):
        with pytest.raises(f.error):
            f.matchTemplate(bad, templ, f.TM_CCORR)
        with pytest.raises(f.error):
            f.matchTemplate(img, bad, f.TM_CCORR)
    for method in (-1, 6, 7, None, 2.5):
        with pytest.raises(f.error, match="TM_"):
            f.matchTemplate(img, templ, method)
    for a, b in ((np.zeros((3, 4097), np.uint8), templ), (np.zeros((4097, 4), np.uint8), templ), (np.zeros((300, 300), np.uint8), np.zeros((257, 256), np.uint8)),
                 (np.zeros((300, 300, 4), np.uint8), np.zeros((128, 129, 4), np.uint8))):
        with pytest.raises(f.error):
            f.matchTemplate(a, b, f.TM_CCORR)
    with pytest.raises(ValueError):
        feature.match_template(img, np.zeros((10, 4), np.uint8))
    with pytest.raises((TypeError, ValueError)):
        feature.DeviceCrop(img, 0, 0, 2, 2)


def test_c_refusals_come_from_the_arguments_alone_and_write_nothing():
    """Without a context an admitted call fails too (VP_ERR_INVALID, silently): what tells the refusals apart is the reason they leave in
    vp_last_error(NULL), which an admitted call does not touch."""
    from vision import _vp
    lib = C.CDLL(_vp.LIB_PATH)
    for name in NEW + ["vp_last_error"]:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _vp._SIGS[name]
    src = np.arange(9 * 12, dtype=np.uint8).reshape(9, 12)
    templ = np.arange(12, dtype=np.uint8).reshape(3, 4)
    dst = np.full((7, 12), 77.0, np.float32)
    p = lambda a: a.ctypes.data
    why = lambda: lib.vp_last_error(None).decode()

    def put_marker():
        assert lib.vp_match_template_u8(None, None, 11, 9, 1, p(templ), 4, 3, 0, p(dst)) == _vp.ERR_INVALID
        return why()

    marker = put_marker()
    assert "pointer" in marker

    def admitted(rc):
        assert rc == _vp.ERR_INVALID and why() == marker, why()

    def refused(rc, words):
        assert rc == _vp.ERR_INVALID and words in why(), (words, why())
        assert put_marker() == marker

    def host(w=11, h=9, cn=1, tw=4, th=3, method=0, s=src, t=templ, d=dst):
        return lib.vp_match_template_u8(None, None if s is None else p(s), w, h, cn, None if t is None else p(t), tw, th, method, None if d is None else p(d))

    def dev(stride=12, w=11, h=9, cn=1, tstride=4, tw=4, th=3, method=0, dstride=48, s=src, t=templ, d=dst, doff=0):
        return lib.vp_match_template_dev(None, None if s is None else p(s), stride, w, h, cn, None if t is None else p(t), tstride, tw, th, method,
                                         None if d is None else p(d) + doff, dstride)

    for call in (host, dev):
        for method in range(6):
            admitted(call(method=method))
        admitted(call(tw=11, th=9, **({"tstride": 11} if call is dev else {})))
        refused(call(w=0), "at least 1")
        refused(call(h=-1), "at least 1")
        refused(call(w=4097, **({"stride": 4097} if call is dev else {})), "4096")
        refused(call(h=4097), "4096")
        for cn in (0, 5, -1):
            refused(call(cn=cn), "1 to 4 channels")
        refused(call(tw=0), "template's width and height")
        refused(call(th=0), "template's width and height")
        refused(call(tw=12), "larger than the image")
        refused(call(th=10), "larger than the image")
        for method in (-1, 6):
            refused(call(method=method), "TM_")
        refused(call(s=None), "pointer")
        refused(call(t=None), "pointer")
        refused(call(d=None), "pointer")
    admitted(host(w=4096, h=4096, tw=256, th=256))
    refused(host(w=4096, h=4096, tw=257, th=256), "65536 bytes")
    admitted(host(w=3, h=3, cn=4, tw=3, th=3))
    refused(host(w=400, h=400, cn=4, tw=129, th=128), "65536 bytes")
    admitted(dev(stride=11, dstride=32))
    admitted(dev(stride=30, tstride=9, dstride=36))
    refused(dev(stride=10), "stride is below the row")
    refused(dev(cn=3, w=5, tw=2, tstride=6, dstride=16), "stride is below the row")
    refused(dev(tstride=3), "template's stride")
    refused(dev(dstride=28), "result's stride is below the row")
    refused(dev(dstride=34), "multiple of the element size")
    refused(dev(doff=2), "aligned")
    refused(lib.vp_match_template_dev(None, p(dst), 12, 11, 9, 1, p(templ), 4, 4, 3, 0, p(dst), 48), "overlaps")
    refused(lib.vp_match_template_dev(None, p(src), 12, 11, 9, 1, p(dst), 4, 4, 3, 0, p(dst), 48), "overlaps")
    assert (dst == 77.0).all(), "a result was written without a context"
