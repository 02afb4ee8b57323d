"""CPU suite for the surface of stereo block matching: the C entries are exported by libvp.so, declared in include/vp.h and bound alike;
the plan's candidate rectangle is the restatement's; every refusal is made from the arguments alone, names its reason and writes
nothing (no device needed: the checks come before the context is touched); the Python layer and the facade have the names and refuse
what the statement leaves out; the names that raise keep raising."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import stereo_cases as SC
import stereo_restate as R
from abi_header import _header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vp_stereo_bm_plan", "vp_stereo_bm_u8", "vp_stereo_bm_dev", "vp_stereo_bm_host", "vp_depth_from_disparity_i16", "vp_depth_from_disparity_dev",
       "vp_depth_from_disparity_host"]


def test_symbols_are_exported_declared_and_bound_alike():
    from vision import _vp
    protos = _header_prototypes()
    lib = C.CDLL(_vp.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name) and name in protos and name in _vp._SIGS, name
        assert protos[name][1] == list(_vp._SIGS[name][1]) and protos[name][0] == "int", name
    assert [len(protos[n][1]) for n in NEW] == [8, 12, 15, 14, 7, 9, 8]
    built = open(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "build.py")).read()
    for src in ("vp_stereo.hip", "vp_api_stereo.hip"):
        assert f'"{src}"' in built, f"{src} is not among VP_SOURCES"
        assert os.path.exists(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc", src))
    assert os.path.exists(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc", "vp_stereo_plan.h"))


def test_plan_rectangle_is_the_statements():
    for h in (4, 9, 40):
        for bs in range(5, 22, 2):
            for n in (16, 32):
                for m in (-3, 0, 4):
                    for w in range(1, 81):
                        assert SC.lib_plan(w, h, n, bs, m)["rect"] == R.valid_rect(w, h, n, bs, m), (w, h, n, bs, m)


def test_plan_geometry_fits_the_device():
    for n in range(16, 257, 16):
        for bs in (5, 21):
            for w, h in ((20, 5), (640, 480), (1280, 720), (4096, 4096)):
                p = SC.lib_plan(w, h, n, bs, 0)
                assert p["strip_cols"] in (32, 64) and 256 % p["strip_cols"] == 0 and p["band_rows"] >= 16 and 0 < p["lds_bytes"] <= 65536
                x, y, cw, ch = p["rect"]
                assert p["grid"][0] * p["strip_cols"] >= cw > (p["grid"][0] - 1) * p["strip_cols"] or cw == 0
                assert p["grid"][1] * p["band_rows"] >= ch > (p["grid"][1] - 1) * p["band_rows"] or ch == 0
                assert p["ws_bytes"] >= 2 * w * h
    assert SC.lib_plan(19, 5, 16, 5, 0)["grid"] == (0, 0)


GOOD = dict(w=40, h=12, n=16, bs=5, m=0, c=31, t=10, u=15)


def _bm_calls(lib, left, right, disp, ls, rs, ds, a):
    """the three matcher entries on one argument set (ctx NULL: a call that passed its checks would stop at the context)"""
    tail = (a["w"], a["h"], a["n"], a["bs"], a["m"], a["c"], a["t"], a["u"])
    yield "host", lambda: lib.vp_stereo_bm_host(left, ls, right, rs, *tail, disp, ds)
    yield "dev", lambda: lib.vp_stereo_bm_dev(None, left, ls, right, rs, *tail, disp, ds)
    if ls == rs == a["w"] and ds == 2 * a["w"]:
        yield "u8", lambda: lib.vp_stereo_bm_u8(None, left, right, *tail, disp)


BM_REFUSALS = [
    ("pointer", dict(left=None)), ("pointer", dict(right=None)), ("pointer", dict(disp=None)),
    ("width", dict(w=0)), ("4096", dict(w=4097)), ("height", dict(h=0)), ("4096", dict(h=4097)),
    ("stride", dict(ls=39)), ("stride", dict(rs=39)), ("stride", dict(ds=79)), ("element size", dict(ds=81)),
    ("num_disparities", dict(n=0)), ("num_disparities", dict(n=24)), ("num_disparities", dict(n=272)),
    ("block_size", dict(bs=3)), ("block_size", dict(bs=8)), ("block_size", dict(bs=23)),
    ("min_disparity", dict(m=-129)), ("min_disparity", dict(m=129)),
    ("pre_filter_cap", dict(c=0)), ("pre_filter_cap", dict(c=64)),
    ("texture_threshold", dict(t=-1)), ("uniqueness_ratio", dict(u=-1)), ("uniqueness_ratio", dict(u=101)),
    ("overlaps", dict(alias="left")), ("overlaps", dict(alias="right")),
]


@pytest.mark.parametrize("word,change", BM_REFUSALS, ids=[f"{w}-{'-'.join(f'{k}{v}' for k, v in c.items())}" for w, c in BM_REFUSALS])
def test_matcher_refusals_name_the_reason_and_write_nothing(word, change):
    from vision import _vp
    lib = _vp.lib()
    a = dict(GOOD, **{k: v for k, v in change.items() if k in GOOD})
    buf = np.full(4097 * 16, 0x5A, np.uint8)                     # room for every size tried; one buffer so that aliasing can be arranged
    left, right, disp = buf[:2048], buf[2048:4096], buf[8192:]
    ptrs = dict(left=left.ctypes.data, right=right.ctypes.data, disp=disp.ctypes.data)
    for k in ("left", "right", "disp"):
        if k in change:
            ptrs[k] = None
    if "alias" in change:
        ptrs["disp"] = ptrs[change["alias"]] + 2 * a["w"]        # the result starts inside an input
    ls, rs, ds = change.get("ls", a["w"]), change.get("rs", a["w"]), change.get("ds", 2 * a["w"])
    ran = 0
    for form, call in _bm_calls(lib, ptrs["left"], ptrs["right"], ptrs["disp"], ls, rs, ds, a):
        assert call() == _vp.ERR_INVALID, form
        assert word in lib.vp_last_error(None).decode(), (form, lib.vp_last_error(None))
        ran += 1
    assert ran >= 2 and np.all(buf == 0x5A)
    if set(change) <= {"w", "h", "n", "bs", "m"}:                # the plan refuses the same geometry
        rect, geom, ws = (C.c_int32 * 4)(*[7] * 4), (C.c_int32 * 5)(*[7] * 5), C.c_size_t(7)
        assert lib.vp_stereo_bm_plan(a["w"], a["h"], a["n"], a["bs"], a["m"], rect, C.byref(ws), geom) == _vp.ERR_INVALID
        assert word in lib.vp_last_error(None).decode() and list(rect) == [7] * 4 and list(geom) == [7] * 5 and ws.value == 7


DEPTH_REFUSALS = [("pointer", dict(disp=None)), ("pointer", dict(depth=None)), ("width", dict(w=0)), ("4096", dict(h=4097)), ("stride", dict(ss=78)),
                  ("element size", dict(ss=81)), ("stride", dict(ds=156)), ("element size", dict(ds=162)), ("overlaps", dict(alias=True))]


@pytest.mark.parametrize("word,change", DEPTH_REFUSALS, ids=[f"{w}-{'-'.join(f'{k}{v}' for k, v in c.items())}" for w, c in DEPTH_REFUSALS])
def test_depth_refusals_name_the_reason_and_write_nothing(word, change):
    from vision import _vp
    lib = _vp.lib()
    w, h = change.get("w", 40), change.get("h", 12)
    buf = np.full(4097 * 512, 0x5A, np.uint8)
    disp = None if "disp" in change else buf.ctypes.data
    depth = None if "depth" in change else buf.ctypes.data + (40 if "alias" in change else 4097 * 256)
    ss, ds = change.get("ss", 80), change.get("ds", 160)
    calls = [lambda: lib.vp_depth_from_disparity_host(disp, ss, w, h, 500.0, 0.1, depth, ds),
             lambda: lib.vp_depth_from_disparity_dev(None, disp, ss, w, h, 500.0, 0.1, depth, ds)]
    if ss == 80 and ds == 160:
        calls.append(lambda: lib.vp_depth_from_disparity_i16(None, disp, w, h, 500.0, 0.1, depth))
    for call in calls:
        assert call() == _vp.ERR_INVALID
        assert word in lib.vp_last_error(None).decode(), lib.vp_last_error(None)
    assert np.all(buf == 0x5A)


def test_an_image_without_candidates_is_no_error():
    left, right = SC.shifted_pair(5, 19, 1)
    out = SC.host_disparity(left, right, num_disparities=16, block_size=5)
    assert np.all(out == -16)


def test_python_names_and_signatures():
    from vision.utils import stereo
    sig = lambda fn: [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    matcher = [("num_disparities", 64), ("block_size", 15), ("min_disparity", 0), ("pre_filter_cap", 31), ("texture_threshold", 10), ("uniqueness_ratio", 15)]
    assert sig(stereo.disparity) == [("left", E), ("right", E)] + matcher
    assert sig(stereo.depth_from_disparity) == [("disp16", E), ("focal_px", E), ("baseline_m", E)]
    assert [n for n, _ in sig(stereo.stereo_depth)] == ["left", "right", "focal_px", "baseline_m", "matcher"]
    assert sig(stereo.invalid_disparity) == [("min_disparity", 0)] and sig(stereo.valid_rect) == [("w", E), ("h", E)] + matcher[:3]
    assert stereo.invalid_disparity(0) == -16 and stereo.invalid_disparity(4) == 48
    assert stereo.valid_rect(640, 480) == R.valid_rect(640, 480) == (70, 7, 563, 466)
    assert stereo.valid_rect(19, 5, 16, 5) == (0, 0, 0, 0)
    img = np.zeros((20, 40), np.uint8)
    for bad in (dict(num_disparities=24), dict(num_disparities=272), dict(block_size=4), dict(block_size=23), dict(min_disparity=129), dict(pre_filter_cap=0),
                dict(texture_threshold=-1), dict(uniqueness_ratio=101)):
        with pytest.raises(ValueError):
            stereo.disparity(img, img, **bad)
    with pytest.raises(ValueError):
        stereo.disparity(img, img[:, :30])
    with pytest.raises(TypeError):
        stereo.disparity(img.astype(np.float32), img)
    with pytest.raises(TypeError):
        stereo.depth_from_disparity(img, 500.0, 0.1)
    with pytest.raises(TypeError):
        stereo.stereo_depth(img, img, 500.0, 0.1, speckle_window_size=3)


def test_facade_surface_and_raises():
    from vision import cv2_facade as f
    sig = lambda fn: [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    assert sig(f.StereoBM_create) == [("numDisparities", 0), ("blockSize", 21)]
    bm = f.StereoBM_create()
    assert (bm.getNumDisparities(), bm.getBlockSize(), bm.getMinDisparity(), bm.getPreFilterCap(), bm.getTextureThreshold(), bm.getUniquenessRatio()) == (64, 21, 0, 31, 10, 15)
    bm = f.StereoBM_create(32, 9)
    for name, value in (("NumDisparities", 48), ("BlockSize", 7), ("MinDisparity", -4), ("PreFilterCap", 20), ("TextureThreshold", 0), ("UniquenessRatio", 5)):
        getattr(bm, "set" + name)(value)
        assert getattr(bm, "get" + name)() == value
    for name, value in (("NumDisparities", 20), ("BlockSize", 6), ("BlockSize", 23), ("MinDisparity", 200), ("PreFilterCap", 64), ("TextureThreshold", -1),
                        ("UniquenessRatio", 101)):
        with pytest.raises(f.error):
            getattr(bm, "set" + name)(value)
    assert (bm.getNumDisparities(), bm.getBlockSize()) == (48, 7)          # a refused value changes nothing
    with pytest.raises(f.error):
        f.StereoBM_create(16, 4)
    # what the statement leaves out keeps cv2's default and refuses everything else
    for name, default, other in (("SpeckleWindowSize", 0, 50), ("SpeckleRange", 0, 2), ("Disp12MaxDiff", -1, 1),
                                 ("PreFilterType", f.StereoBM_PREFILTER_XSOBEL, f.StereoBM_PREFILTER_NORMALIZED_RESPONSE), ("PreFilterSize", 9, 5),
                                 ("ROI1", (0, 0, 0, 0), (1, 1, 5, 5)), ("ROI2", (0, 0, 0, 0), (1, 1, 5, 5))):
        assert getattr(bm, "get" + name)() == default
        getattr(bm, "set" + name)(default)
        with pytest.raises(f.error):
            getattr(bm, "set" + name)(other)
    with pytest.raises(f.error):
        bm.compute(np.zeros((20, 40, 3), np.uint8), np.zeros((20, 40, 3), np.uint8))
    with pytest.raises(f.error):
        bm.compute(np.zeros((20, 40), np.uint8), np.zeros((20, 41), np.uint8))
    assert not hasattr(f, "StereoSGBM_create") and not hasattr(f, "StereoSGBM")
    mod = f.install()
    assert hasattr(mod, "StereoBM_create") and not hasattr(mod, "StereoSGBM_create")


def test_the_names_that_raise_keep_raising():
    from vision import cv2_facade as f
    from vision.utils import feature
    for name in ("find_corners", "find_circles", "find_line_segments"):
        with pytest.raises(Exception):
            getattr(feature, name)(np.zeros((4, 4), np.uint8))
    with pytest.raises(Exception):
        f.fitEllipse(np.zeros((5, 1, 2), np.int32))
