"""CPU suite for the surface of the colour-histogram family (cv2.calcHist, calcBackProject, meanShift, CamShift): the six C entries are
exported by libvp.so and declared in include/vp.h with the prototypes vision/_vp.py binds; the units are built; the plan's limits come
from the LDS of a gfx950 compute unit; the facade has the names and cv2's constants; every refusal comes from the arguments alone -
VP_ERR_INVALID / VP_ERR_UNSUPPORTED with its reason from the C entries, cv2_facade.error from the facade, no device needed, nothing
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
NEW = ["vp_calc_hist_u8", "vp_calc_hist_dev", "vp_back_project_u8", "vp_back_project_dev", "vp_back_project_table_dev", "vp_mean_shift_dev"]


def test_hist_symbols_are_exported_declared_and_bound_alike():
    from vision import _vp
    protos = _header_prototypes()
    lib = C.CDLL(_vp.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name) and name in protos and name in _vp._SIGS, name
        assert protos[name][0] == "int" and protos[name][1] == _vp._SIGS[name][1] and _vp._SIGS[name][0] is C.c_int, name
    assert [len(protos[n][1]) for n in NEW] == [13, 17, 12, 14, 13, 11]
    built = open(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "build.py")).read()
    for src in ("vp_hist.hip", "vp_api_hist.hip"):
        assert f'"{src}"' in built, f"{src} is not among VP_SOURCES"
        assert os.path.exists(os.path.join(CSRC, src))
    assert os.path.exists(os.path.join(CSRC, "vp_hist_plan.h"))
    assert len(header_options()) == 11, "the histogram family adds no option"


def test_plan_limits_come_from_the_lds_of_a_compute_unit():
    plan = open(os.path.join(CSRC, "vp_hist_plan.h")).read()
    num = lambda n: int(re.search(r"#define " + n + r" (\d+)", plan).group(1))
    lds, tabs, bins, table = num("HS_LDS_BYTES"), num("HS_TAB_LDS_BYTES"), num("HS_HIST_LDS_BINS"), num("HS_BP_LDS_BYTES")
    assert lds == 160 * 1024 and tabs == 3 * 256 * 4 and num("HS_MAX_SIDE") == 4096 and num("HS_MAX_SIZE") == 256 and num("HS_MAX_DIMS") == 3
    assert tabs + 4 * bins <= lds and tabs + (table + 3) // 4 * 4 <= lds
    assert 32 ** 3 <= bins < 180 * 256, "32^3 counters fit a block, 180 x 256 do not"
    assert 256 * 256 <= table < 64 ** 3 and 180 * 256 <= table, "both typical tables and 256 x 256 fit, 64^3 does not"

    def three_sizes(n):
        return any(n % a == 0 and any((n // a) % b == 0 and (n // a) // b <= 256 for b in range(a, 257)) for a in range(1, 257))
    for limit in (bins, table):                         # a test can stand one below, at and one above either limit
        assert all(three_sizes(limit + d) for d in (-1, 0, 1)), limit
    kernels = open(os.path.join(CSRC, "vp_hist.hip")).read()
    assert '#include "vp_hist_plan.h"' in kernels and "P.lds_bytes" in kernels and "__ballot" in kernels and "__launch_bounds__(HS_THREADS)" in kernels
    assert "cooperative" not in kernels and "grid.sync" not in kernels, "mean shift uses no grid-wide barrier"


def test_facade_names_signatures_and_constants():
    from vision import cv2_facade as f
    from vision.utils import color, feature
    sig = lambda fn: [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(f.calcHist) == [("images", E), ("channels", E), ("mask", E), ("histSize", E), ("ranges", E), ("hist", None), ("accumulate", False)]
    assert sig(f.calcBackProject) == [("images", E), ("channels", E), ("hist", E), ("ranges", E), ("scale", E), ("dst", None)]
    assert sig(f.meanShift) == [("probImage", E), ("window", E), ("criteria", E)] == sig(f.CamShift)
    assert [n for n, _ in sig(f.normalize)][:5] == ["src", "dst", "alpha", "beta", "norm_type"]
    assert (f.NORM_INF, f.NORM_L1, f.NORM_L2, f.NORM_MINMAX) == (1, 2, 4, 32)
    assert (f.TERM_CRITERIA_COUNT, f.TERM_CRITERIA_MAX_ITER, f.TERM_CRITERIA_EPS) == (1, 1, 2)
    assert sig(color.color_histogram) == [("mat", E), ("channels", E), ("hist_size", E), ("ranges", E), ("mask", None)]
    assert sig(color.back_project) == [("mat", E), ("channels", E), ("hist", E), ("ranges", E), ("scale", 1.0)]
    assert sig(color.HistModel.from_patch) == [("mat", E), ("channels", E), ("hist_size", E), ("ranges", E), ("mask", None), ("top", 255.0)]
    assert sig(color.normalize_hist)[:2] == [("hist", E), ("top", 255.0)] and hasattr(color.HistModel, "apply")
    assert sig(feature.mean_shift) == [("prob", E), ("window", E), ("max_iter", 10), ("eps", 1.0)] == sig(feature.cam_shift)
    assert sig(feature.mean_shift_many) == [("prob", E), ("windows", E), ("max_iter", 10), ("eps", 1.0)]
    mod = f.install()
    for name in ("calcHist", "calcBackProject", "meanShift", "CamShift", "normalize", "NORM_MINMAX"):
        assert hasattr(mod, name), name
    for name in ("find_corners", "find_circles", "find_line_segments"):                 # the names that raise keep raising
        with pytest.raises(Exception):
            getattr(feature, name)(np.zeros((4, 4), np.uint8))


def test_normalize_is_the_statement_and_refuses_the_rest():
    import hist_restate as R
    from vision import cv2_facade as f
    from vision.utils import color
    h = np.array([[2, 4], [3, 10]], np.float32)
    assert color.normalize_hist(h).tobytes() == R.normalize_hist(h).tobytes() == np.array([[0, 63.75], [31.875, 255]], np.float32).tobytes()
    r = np.random.default_rng(3).integers(0, 5000, (7, 9)).astype(np.float32)
    for top, low in ((255.0, 0.0), (1.0, 0.0), (100.0, 7.5)):
        assert color.normalize_hist(r, top, low).tobytes() == R.normalize_hist(r, top, low).tobytes()
        assert f.normalize(r, None, low, top, f.NORM_MINMAX).tobytes() == R.normalize_hist(r, top, low).tobytes()
    assert f.normalize(r, None, 255, 0, f.NORM_MINMAX).tobytes() == R.normalize_hist(r).tobytes()          # alpha and beta in either order
    dst = np.zeros_like(r)
    assert f.normalize(r, dst, 0, 255, f.NORM_MINMAX) is dst and dst.tobytes() == R.normalize_hist(r).tobytes()
    assert color.fold_hist(np.array([1, 3, 5, 7, 600, -3, np.nan], np.float32), 0.5).tolist() == [0, 2, 2, 4, 255, 0, 0]
    for bad in (lambda: f.normalize(r, None, 0, 255, f.NORM_L2), lambda: f.normalize(r, None, 0, 255), lambda: f.normalize(r.astype(np.float64), None, 0, 255, f.NORM_MINMAX),
                lambda: f.normalize(r, None, 0, 255, f.NORM_MINMAX, mask=np.ones(r.shape, np.uint8)), lambda: f.normalize(r.astype(np.uint8), None, 0, 255, f.NORM_MINMAX),
                lambda: f.normalize(np.array([np.nan], np.float32), None, 0, 255, f.NORM_MINMAX)):
        with pytest.raises(f.error):
            bad()


def test_facade_refuses_what_is_outside_the_contract_before_it_needs_a_device():
    from vision import cv2_facade as f
    bgr, grey = np.zeros((9, 11, 3), np.uint8), np.zeros((9, 11), np.uint8)
    hist2 = np.zeros((4, 5), np.float32)
    crit = (f.TERM_CRITERIA_EPS | f.TERM_CRITERIA_COUNT, 10, 1)

    def refused(call, *words):
        with pytest.raises(f.error) as e:
            call()
        assert all(w in str(e.value) for w in words), str(e.value)

    refused(lambda: f.calcHist([bgr], [0], None, [8], [0, 256], None, True), "accumulate")
    refused(lambda: f.calcHist([bgr, bgr], [0], None, [8], [0, 256]), "one image")
    refused(lambda: f.calcHist(bgr, [0], None, [8], [0, 256]), "one image")
    refused(lambda: f.calcHist([], [0], None, [8], [0, 256]), "one image")
    refused(lambda: f.calcHist([bgr.astype(np.float32)], [0], None, [8], [0, 256]), "uint8")
    refused(lambda: f.calcHist([bgr.astype(np.uint16)], [0], None, [8], [0, 256]), "uint8")
    refused(lambda: f.calcHist([bgr], [], None, [], []), "1 to 3 dimensions")
    refused(lambda: f.calcHist([np.zeros((9, 11, 4), np.uint8)], [0, 1, 2, 3], None, [4] * 4, [0, 256] * 4), "1 to 3 dimensions")
    refused(lambda: f.calcHist([bgr], [3], None, [8], [0, 256]), "channel index")
    refused(lambda: f.calcHist([bgr], [-1], None, [8], [0, 256]), "channel index")
    refused(lambda: f.calcHist([grey], [1], None, [8], [0, 256]), "channel index")
    refused(lambda: f.calcHist([bgr], [0], None, [0], [0, 256]), "1 to 256")
    refused(lambda: f.calcHist([bgr], [0], None, [257], [0, 256]), "1 to 256")
    refused(lambda: f.calcHist([bgr], [0, 1], None, [8], [0, 256, 0, 256]), "one histogram size per dimension")
    refused(lambda: f.calcHist([bgr], [0], None, [8], [5, 5]), "low < high")
    refused(lambda: f.calcHist([bgr], [0], None, [8], [9, 1]), "low < high")
    refused(lambda: f.calcHist([bgr], [0], None, [8], [0, float("inf")]), "low < high")
    refused(lambda: f.calcHist([bgr], [0], None, [3], [0, 10, 50, 256]), "non-uniform")
    refused(lambda: f.calcHist([bgr], [0, 1], None, [3, 3], [[0, 10, 256], [0, 256]]), "non-uniform")
    refused(lambda: f.calcHist([np.zeros((3, 4097), np.uint8)], [0], None, [8], [0, 256]), "4096")
    refused(lambda: f.calcHist([np.zeros((4097, 3), np.uint8)], [0], None, [8], [0, 256]), "4096")
    refused(lambda: f.calcHist([bgr], [0], np.ones((9, 10), np.uint8), [8], [0, 256]), "size of the image")
    refused(lambda: f.calcHist([bgr], [0], np.ones((9, 11), np.float32), [8], [0, 256]), "mask")
    refused(lambda: f.calcBackProject([bgr, bgr], [0, 1], hist2, [0, 180, 0, 256], 1), "one image")
    refused(lambda: f.calcBackProject([bgr], [0, 1], hist2.astype(np.float64), [0, 180, 0, 256], 1), "float32")
    refused(lambda: f.calcBackProject([bgr], [0, 1], np.zeros(4, np.float32), [0, 180, 0, 256], 1), "per dimension")
    refused(lambda: f.calcBackProject([bgr], [0, 1, 2], hist2, [0, 180, 0, 256, 0, 256], 1), "")
    refused(lambda: f.calcBackProject([bgr], [0, 3], hist2, [0, 180, 0, 256], 1), "channel index")
    refused(lambda: f.calcBackProject([bgr], [0, 1], hist2, [0, 180, 7, 7], 1), "low < high")
    refused(lambda: f.calcBackProject([bgr], [0, 1], hist2, [0, 180, 0, 256], float("nan")), "finite")
    refused(lambda: f.calcBackProject([np.zeros((3, 4097, 3), np.uint8)], [0, 1], hist2, [0, 180, 0, 256], 1), "4096")
    for call in (f.meanShift, f.CamShift):
        refused(lambda: call(grey, (0, 0, 0, 3), crit), "non-positive")
        refused(lambda: call(grey, (0, 0, 3, -1), crit), "non-positive")
        refused(lambda: call(grey, (11, 0, 3, 3), crit), "empty inside the image")
        refused(lambda: call(grey, (-3, 2, 3, 3), crit), "empty inside the image")
        refused(lambda: call(grey, (0, 0, 3), crit), "four integers")
        refused(lambda: call(bgr, (0, 0, 3, 3), crit), "single-channel")
        refused(lambda: call(grey.astype(np.float32), (0, 0, 3, 3), crit), "uint8")
        refused(lambda: call(np.zeros((3, 4097), np.uint8), (0, 0, 3, 3), crit), "4096")
        refused(lambda: call(grey, (0, 0, 3, 3), None), "criteria")
        refused(lambda: call(grey, (0, 0, 3, 3), (f.TERM_CRITERIA_COUNT, 100001, 1)), "100000")


def test_c_refusals_come_from_the_arguments_alone_and_write_nothing():
    """Without a context an admitted call fails too (VP_ERR_INVALID, silently): what tells the refusals apart is the reason they leave in
    vp_last_error(NULL), which an admitted call does not touch."""
    from vision import _vp
    lib = C.CDLL(_vp.LIB_PATH)
    for name in NEW + ["vp_last_error"]:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _vp._SIGS[name]
    src = np.arange(9 * 36, dtype=np.uint8).reshape(9, 36)               # 9 rows of 12 pixels of 3 channels (or 36 of one)
    mask = np.ones((9, 12), np.uint8)
    bits = np.zeros(16, np.uint64)
    hist = np.full(4 * 5 * 6, 7.0, np.float32)
    counts = np.full(4 * 5 * 6, 77, np.uint32)
    table = np.full(4 * 5 * 6, 9, np.uint8)
    dst = np.full((9, 12), 77, np.uint8)
    out = np.full((3, 5), 77, np.int32)
    p = lambda a, off=0: None if a is None else a.ctypes.data + off
    why = lambda: lib.vp_last_error(None).decode()
    i32 = lambda *v: np.array(v, np.int32)
    f64 = lambda *v: np.array(v, np.float64)

    def put_marker():
        assert lib.vp_mean_shift_dev(None, None, 12, 12, 9, None, 1, 10, 1.0, None, None) == _vp.ERR_INVALID
        return why()

    marker = put_marker()
    assert "pointer" in marker

    def admitted(rc):
        assert rc == _vp.ERR_INVALID and why() == marker, why()

    def refused(rc, words, code=_vp.ERR_INVALID):
        assert rc == code and words in why(), (words, why())
        assert put_marker() == marker

    def desc(dims=3, ch=(0, 1, 2), sz=(4, 5, 6), rg=(0, 180, 0, 256, 10.5, 200.25)):
        keep = (i32(*ch), i32(*sz), f64(*rg))
        return (dims, p(keep[0]), p(keep[1]), p(keep[2])), keep

    def hist_u8(w=12, h=9, cn=3, m=None, mw=0, mh=0, s=src, o=hist, **d):
        a, keep = desc(**d)
        return lib.vp_calc_hist_u8(None, p(s), w, h, cn, *a, p(m), mw, mh, p(o))

    def hist_dev(stride=36, w=12, h=9, cn=3, m=None, ms=0, mw=0, mh=0, b=None, boff=0, s=src, cd=counts, ch_=None, cdoff=0, **d):
        a, keep = desc(**d)
        return lib.vp_calc_hist_dev(None, p(s), stride, w, h, cn, *a, p(m), ms, mw, mh, p(b, boff), p(cd, cdoff), p(ch_))

    def bp_u8(w=12, h=9, cn=3, scale=1.0, s=src, hh=hist, o=dst, **d):
        a, keep = desc(**d)
        return lib.vp_back_project_u8(None, p(s), w, h, cn, *a, p(hh), scale, p(o))

    def bp_dev(stride=36, w=12, h=9, cn=3, scale=1.0, s=src, hh=hist, hoff=0, o=dst, ds=12, **d):
        a, keep = desc(**d)
        return lib.vp_back_project_dev(None, p(s), stride, w, h, cn, *a, p(hh, hoff), scale, p(o), ds)

    def bp_tab(stride=36, w=12, h=9, cn=3, s=src, t=table, o=dst, ds=12, **d):
        a, keep = desc(**d)
        return lib.vp_back_project_table_dev(None, p(s), stride, w, h, cn, *a, p(t), p(o), ds)

    def shift(stride=12, w=12, h=9, wins=((1, 1, 4, 4), (-2, 3, 5, 9), (11, 8, 1, 1)), n=None, max_iter=10, eps=1.0, s=src, od=out, oh=None, odoff=0):
        wa = None if wins is None else i32(*[v for win in wins for v in win])
        return lib.vp_mean_shift_dev(None, p(s), stride, w, h, p(wa), len(wins) if n is None else n, max_iter, eps, p(od, odoff), p(oh))

    described = (hist_u8, hist_dev, bp_u8, bp_dev, bp_tab)
    for call in described:
        admitted(call())
        admitted(call(dims=1, ch=(2,), sz=(256,), rg=(0, 256)))
        admitted(call(dims=2, ch=(1, 1), sz=(1, 120), rg=(-5, 300, 0.5, 0.75)))
        refused(call(dims=0), "1 to 3 dimensions")
        refused(call(dims=4), "1 to 3 dimensions")
        refused(call(ch=(0, 3, 1)), "channel index")
        refused(call(ch=(-1, 0, 1)), "channel index")
        refused(call(cn=1, w=36, ch=(0, 0, 1), **({"stride": 36} if "stride" in inspect.signature(call).parameters else {})), "channel index")
        refused(call(sz=(4, 0, 6)), "1 to 256")
        refused(call(sz=(257, 5, 6)), "1 to 256")
        refused(call(rg=(0, 180, 5, 5, 0, 256)), "low < high")
        refused(call(rg=(0, 180, 0, 256, 9, 1)), "low < high")
        refused(call(rg=(0, float("nan"), 0, 256, 0, 256)), "low < high")
        refused(call(w=4097, **({"stride": 4097 * 3} if "stride" in inspect.signature(call).parameters else {})), "4096")
        refused(call(h=4097), "4096")
        refused(call(w=0), "at least 1")
        refused(call(cn=5), "1 to 4 channels")
        refused(call(cn=0), "1 to 4 channels")
        refused(call(s=None), "pointer")
    for call in (hist_dev, bp_dev, bp_tab):
        refused(call(stride=35), "stride is below the row")
    # masks
    admitted(hist_u8(m=mask, mw=12, mh=9))
    admitted(hist_dev(m=mask, ms=12, mw=12, mh=9))
    admitted(hist_dev(m=mask, ms=40, mw=12, mh=9, b=bits))
    admitted(hist_dev(b=bits, mw=12, mh=9))
    refused(hist_u8(m=mask, mw=11, mh=9), "size of the image")
    refused(hist_u8(m=mask, mw=12, mh=10), "size of the image")
    refused(hist_dev(m=mask, ms=12, mw=9, mh=12), "size of the image")
    refused(hist_dev(b=bits, mw=0, mh=0), "size of the image")
    refused(hist_dev(m=mask, ms=11, mw=12, mh=9), "mask's stride")
    refused(hist_dev(b=bits, boff=4, mw=12, mh=9), "8-byte aligned")
    # results
    admitted(hist_dev(cd=None, ch_=counts))
    refused(hist_dev(cd=None, ch_=None), "pointer")
    refused(hist_dev(cdoff=2), "aligned")
    refused(hist_u8(o=None), "pointer")
    held = desc()
    refused(lib.vp_calc_hist_dev(None, p(counts), 36, 12, 9, 3, *held[0], None, 0, 0, 0, None, p(counts), None), "overlap")
    for call in (bp_u8, bp_dev):
        refused(call(scale=float("inf")), "finite")
        refused(call(scale=float("nan")), "finite")
        refused(call(hh=None), "pointer")
        refused(call(o=None), "pointer")
    refused(bp_tab(t=None), "pointer")
    refused(bp_dev(hoff=2), "aligned")
    for call in (bp_dev, bp_tab):
        refused(call(ds=11), "result's stride")
        admitted(call(ds=12))
        refused(call(s=dst, stride=12, cn=1, ch=(0, 0, 0)), "overlaps the image")          # source and destination are one buffer
    refused(bp_tab(t=dst, sz=(4, 5, 5)), "overlaps the histogram or the table")
    refused(bp_dev(hh=dst.view(np.float32), sz=(3, 3, 3)), "overlaps the histogram or the table")
    # mean shift
    admitted(shift())
    admitted(shift(od=None, oh=out))
    admitted(shift(max_iter=-3, eps=-1.0))
    admitted(shift(max_iter=100000))
    refused(shift(max_iter=100001), "100000", _vp.ERR_UNSUPPORTED)
    refused(shift(wins=((1, 1, 0, 4),)), "non-positive")
    refused(shift(wins=((1, 1, 4, 4), (1, 1, 4, -4))), "non-positive")
    refused(shift(wins=((12, 0, 4, 4),)), "empty inside the image")
    refused(shift(wins=((1, 1, 4, 4), (0, -4, 4, 4))), "empty inside the image")
    refused(shift(wins=((2147483647, 2147483647, 2147483647, 2147483647),)), "empty inside the image")
    refused(shift(n=0), "1 to 4096 windows")
    refused(shift(n=4097), "1 to 4096 windows")
    refused(shift(stride=11), "stride is below the row")
    refused(shift(w=4097, stride=4097), "4096")
    refused(shift(wins=None, n=1), "pointer")
    refused(shift(od=None, oh=None), "pointer")
    refused(shift(odoff=2), "aligned")
    refused(lib.vp_mean_shift_dev(None, p(out), 4, 4, 3, p(i32(0, 0, 2, 2)), 1, 10, 1.0, p(out), None), "overlaps")
    assert (dst == 77).all() and (counts == 77).all() and (out == 77).all() and (hist == 7.0).all(), "a result was written without a context"
