"""CPU suite for the surface of the speckle filter and the surface normals: the C entries are exported, declared and bound alike; the
plan is monotone and its workspace covers labels and counts; every refusal is made from the arguments alone, names its argument and
writes nothing (no device needed: the checks come before the context is touched); the Python layer and the facade have the names, the
defaults and the TypeError / ValueError split; what the stereo tests pin still holds."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import speckle_cases as SC
import speckle_restate as R
from abi_header import _header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vp_filter_speckles_plan", "vp_filter_speckles_i16", "vp_filter_speckles_dev", "vp_filter_speckles_host", "vp_normals_from_depth_f32",
       "vp_normals_from_depth_dev", "vp_normals_from_depth_host"]


def test_symbols_are_exported_declared_and_bound_alike():
    from vision import _vp
    protos = _header_prototypes()
    lib = C.CDLL(_vp.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name) and name in protos and name in _vp._SIGS, name
        assert protos[name][1] == list(_vp._SIGS[name][1]) and protos[name][0] == "int", name
    assert [len(protos[n][1]) for n in NEW] == [4, 8, 10, 9, 10, 12, 11]
    built = open(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "build.py")).read()
    for src in ("vp_speckle.hip", "vp_api_speckle.hip"):
        assert f'"{src}"' in built, f"{src} is not among VP_SOURCES"
        assert os.path.exists(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc", src))
    assert os.path.exists(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc", "vp_speckle_plan.h"))


def test_plan_is_monotone_and_covers_labels_and_counts():
    T = SC.tile()
    assert T >= 8 and T % 4 == 0
    last = 0
    for side in (1, 2, T - 1, T, T + 1, 2 * T, 2 * T + 1, 640, 1280, 4095, 4096):
        p = SC.lib_plan(side, side)
        assert p["tile_w"] == p["tile_h"] == T and 0 < p["lds_bytes"] <= 65536
        assert p["grid"] == ((side + T - 1) // T, (side + T - 1) // T)
        assert p["ws_bytes"] >= 8 * side * side and p["ws_bytes"] >= last                     # an int32 label and an int32 count per pixel
        last = p["ws_bytes"]
    assert SC.lib_plan(1, 1)["ws_bytes"] >= 8 and SC.lib_plan(4096, 4096)["ws_bytes"] >= 8 * 4096 * 4096
    assert SC.lib_plan(4096, 4096)["ws_bytes"] < 9 * 4096 * 4096                              # about 8 B per pixel, not more
    assert SC.lib_plan(1280, 720)["grid"] == ((1280 + T - 1) // T, (720 + T - 1) // T)
    assert SC.lib_plan(3 * T, T + 1)["ws_bytes"] <= SC.lib_plan(3 * T, T + 2)["ws_bytes"] <= SC.lib_plan(3 * T + 1, T + 2)["ws_bytes"]


GOOD = dict(w=40, h=12, nv=-16, size=5, diff=2)

SPECKLE_REFUSALS = [
    ("pointer", dict(src=None)), ("pointer", dict(dst=None)),
    ("width", dict(w=0)), ("4096", dict(w=4097)), ("height", dict(h=0)), ("4096", dict(h=4097)),
    ("stride", dict(ss=78)), ("element size", dict(ss=81)), ("stride", dict(ds=79)), ("element size", dict(ds=83)),
    ("max_diff", dict(diff=-1)), ("max_diff", dict(diff=65536)),
    ("max_speckle_size", dict(size=-1)), ("max_speckle_size", dict(size=40 * 12 + 1)),
    ("new_val", dict(nv=32768)), ("new_val", dict(nv=-32769)),
    ("overlaps", dict(alias=2)), ("overlaps", dict(alias=80)), ("overlaps", dict(alias=0, ds=160)),
]


@pytest.mark.parametrize("word,change", SPECKLE_REFUSALS, ids=[f"{w}-{'-'.join(f'{k}{v}' for k, v in c.items())}" for w, c in SPECKLE_REFUSALS])
def test_speckle_refusals_name_the_argument_and_write_nothing(word, change):
    from vision import _vp
    lib = _vp.lib()
    a = dict(GOOD, **{k: v for k, v in change.items() if k in GOOD})
    buf = np.full(4097 * 32, 0x5A, np.uint8)
    src = None if "src" in change else buf.ctypes.data
    dst = None if "dst" in change else buf.ctypes.data + (change["alias"] if "alias" in change else 4097 * 16)
    ss, ds = change.get("ss", 2 * a["w"]), change.get("ds", 2 * a["w"])
    tail = (a["w"], a["h"], a["nv"], a["size"], a["diff"])
    calls = [lambda: lib.vp_filter_speckles_host(src, ss, *tail, dst, ds), lambda: lib.vp_filter_speckles_dev(None, src, ss, *tail, dst, ds)]
    if ss == ds == 2 * a["w"]:
        calls.append(lambda: lib.vp_filter_speckles_i16(None, src, *tail, dst))
    for call in calls:
        assert call() == _vp.ERR_INVALID
        assert word in lib.vp_last_error(None).decode(), lib.vp_last_error(None)
    assert np.all(buf == 0x5A)
    if set(change) <= {"w", "h"}:                                                             # the plan refuses the same geometry
        geom, ws = (C.c_int32 * 5)(*[7] * 5), C.c_size_t(7)
        assert lib.vp_filter_speckles_plan(a["w"], a["h"], C.byref(ws), geom) == _vp.ERR_INVALID
        assert word in lib.vp_last_error(None).decode() and list(geom) == [7] * 5 and ws.value == 7


def test_plan_refuses_missing_pointers():
    from vision import _vp
    lib = _vp.lib()
    geom, ws = (C.c_int32 * 5)(), C.c_size_t()
    assert lib.vp_filter_speckles_plan(8, 8, None, geom) == _vp.ERR_INVALID and lib.vp_filter_speckles_plan(8, 8, C.byref(ws), None) == _vp.ERR_INVALID


def test_exact_dst_equals_src_is_accepted_by_the_host_form():
    from vision import _vp
    img = SC.noise(12, 40, (7, 8, 20), 6, holes=0.05)
    want = R.filter_speckles(img, -16, 5, 0)
    work = img.copy()
    assert _vp.lib().vp_filter_speckles_host(work.ctypes.data, 80, 40, 12, -16, 5, 0, work.ctypes.data, 80) == _vp.OK
    assert np.array_equal(work, want) and not np.array_equal(work, img)
    # the device forms pass the same check: with no context they stop at the context, not at the overlap
    assert _vp.lib().vp_filter_speckles_dev(None, work.ctypes.data, 80, 40, 12, -16, 5, 0, work.ctypes.data, 80) == _vp.ERR_INVALID
    assert "overlaps" not in _vp.lib().vp_last_error(None).decode()


NORMALS_REFUSALS = [
    ("pointer", dict(depth=None)), ("pointer", dict(normals=None)), ("width", dict(w=0)), ("4096", dict(w=4097)), ("height", dict(h=0)), ("4096", dict(h=4097)),
    ("stride", dict(zs=156)), ("element size", dict(zs=162)), ("stride", dict(ns=476)), ("element size", dict(ns=482)),
    ("focal_px", dict(f=float("nan"))), ("focal_px", dict(f=float("inf"))), ("focal_px", dict(f=0.0)), ("focal_px", dict(f=-500.0)),
    ("cx", dict(cx=float("nan"))), ("cy", dict(cy=float("inf"))), ("max_jump_m", dict(jump=float("nan"))), ("overlaps", dict(alias=True)),
]


@pytest.mark.parametrize("word,change", NORMALS_REFUSALS, ids=[f"{w}-{'-'.join(f'{k}{v}' for k, v in c.items())}" for w, c in NORMALS_REFUSALS])
def test_normals_refusals_name_the_argument_and_write_nothing(word, change):
    from vision import _vp
    lib = _vp.lib()
    w, h = change.get("w", 40), change.get("h", 12)
    buf = np.full(4097 * 64, 0x5A, np.uint8)
    depth = None if "depth" in change else buf.ctypes.data
    normals = None if "normals" in change else buf.ctypes.data + (40 if "alias" in change else 4097 * 32)
    zs, ns = change.get("zs", 160), change.get("ns", 480)
    mid = (change.get("f", 500.0), change.get("cx", 19.5), change.get("cy", 5.5), change.get("jump", 0.0), 0)
    calls = [lambda: lib.vp_normals_from_depth_host(depth, zs, w, h, *mid, normals, ns), lambda: lib.vp_normals_from_depth_dev(None, depth, zs, w, h, *mid, normals, ns)]
    if zs == 160 and ns == 480:
        calls.append(lambda: lib.vp_normals_from_depth_f32(None, depth, w, h, *mid, normals))
    for call in calls:
        assert call() == _vp.ERR_INVALID
        assert word in lib.vp_last_error(None).decode(), lib.vp_last_error(None)
    assert np.all(buf == 0x5A)


def test_python_names_signatures_and_the_error_split():
    from vision.utils import stereo
    sig = lambda fn: [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(stereo.filter_speckles) == [("disp16", E), ("max_speckle_size", E), ("max_diff", E), ("new_val", None)]
    assert sig(stereo.normals_from_depth) == [("depth", E), ("focal_px", E), ("cx", None), ("cy", None), ("max_jump_m", None), ("encode", False)]
    assert sig(stereo.stereo_planes)[:-1] == [("left", E), ("right", E), ("focal_px", E), ("baseline_m", E), ("cx", None), ("cy", None), ("speckle_window_size", 100),
                                              ("speckle_range", 2), ("max_jump_m", None)]
    assert sig(stereo.stereo_planes)[-1][0] == "matcher" and "nothing here measured them" in " ".join(stereo.stereo_planes.__doc__.split())
    disp = np.zeros((6, 8), np.int16)
    for bad in (disp.astype(np.int32), disp.astype(np.uint8), disp[None], np.zeros((0, 4), np.int16), [[1, 2]]):
        with pytest.raises(TypeError):
            stereo.filter_speckles(bad, 3, 1)
    for args in ((3.0, 1), (3, 1.5), (True, 1), (3, 1, 2.0)):
        with pytest.raises(TypeError):
            stereo.filter_speckles(disp, *args)
    for args in ((-1, 1), (49, 1), (3, -1), (3, 65536), (3, 1, 32768), (3, 1, -32769)):
        with pytest.raises(ValueError):
            stereo.filter_speckles(disp, *args)
    depth = np.ones((6, 8), np.float32)
    for bad in (depth.astype(np.float64), disp, depth[None], np.zeros((0, 4), np.float32)):
        with pytest.raises(TypeError):
            stereo.normals_from_depth(bad, 500.0)
    for kw in (dict(focal_px=float("nan")), dict(focal_px=float("inf")), dict(focal_px=0.0), dict(focal_px=500.0, cx=float("nan")),
               dict(focal_px=500.0, max_jump_m=float("nan"))):
        with pytest.raises(ValueError):
            stereo.normals_from_depth(depth, **kw)
    img = np.zeros((20, 40), np.uint8)
    with pytest.raises(ValueError):
        stereo.stereo_planes(img, img, 500.0, 0.1, speckle_window_size=-1)
    with pytest.raises(ValueError):
        stereo.stereo_planes(img, img, 500.0, 0.1, speckle_range=-1)
    with pytest.raises(ValueError):
        stereo.stereo_planes(img, img, float("nan"), 0.1)
    with pytest.raises(ValueError):
        stereo.stereo_planes(img, img, 500.0, 0.1, block_size=4)
    with pytest.raises(TypeError):
        stereo.stereo_planes(img, img, 500.0, 0.1, speckle_window_size=2.5)
    with pytest.raises(TypeError):
        stereo.stereo_planes(img, img, 500.0, 0.1, bogus=1)


def test_facade_filter_speckles_is_cv2s(monkeypatch):
    from vision import cv2_facade as f
    from vision.utils import stereo
    assert list(inspect.signature(f.filterSpeckles).parameters) == ["img", "newVal", "maxSpeckleSize", "maxDiff", "buf"]
    assert inspect.signature(f.filterSpeckles).parameters["buf"].default is None
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.float32), np.zeros((4, 4, 1), np.int16), np.zeros((0, 4), np.int16), [[1, 2]]):
        with pytest.raises(f.error):
            f.filterSpeckles(bad, 0, 3, 1)
    with pytest.raises(f.error):
        f.filterSpeckles(np.zeros((4, 4), np.int16), 0, 17, 1)
    with pytest.raises(f.error):
        f.filterSpeckles(np.zeros((4, 4), np.int16), 0, 3, -1)
    # in place, (img, buf) back: with the device call replaced by the host routine (this is the CPU suite)
    from vision import _vp
    real = _vp.lib()

    class _Lib:
        def __getattr__(self, name):
            return getattr(real, name)

        def vp_filter_speckles_i16(self, ctx, src, w, h, nv, size, diff, dst):
            return real.vp_filter_speckles_host(src, 2 * w, w, h, nv, size, diff, dst, 2 * w)

    class _Ctx:
        handle = None
    monkeypatch.setattr(f._vp, "lib", lambda: _Lib())
    monkeypatch.setattr(f._vp, "default_context", lambda: _Ctx())
    img = SC.noise(9, 14, (7, 8, 20), 1, holes=0.1)
    want = R.filter_speckles(img, -16, 4, 1)
    buf = object()
    got, back = f.filterSpeckles(img, -16, 4, 1, buf)
    assert got is img and back is buf and np.array_equal(img, want)
    wide = np.full((9, 20), 99, np.int16)
    wide[:, 3:17] = SC.noise(9, 14, (7, 8, 20), 1, holes=0.1)
    view = wide[:, 3:17]                                                                       # not contiguous: still in place
    got, back = f.filterSpeckles(view, -16, 4, 1)
    assert got is view and back is None and np.array_equal(wide[:, 3:17], want) and np.all(wide[:, :3] == 99) and np.all(wide[:, 17:] == 99)
    mod = f.install()
    assert hasattr(mod, "filterSpeckles")
    assert stereo.filter_speckles.__doc__ and "cv2.filterSpeckles" in stereo.filter_speckles.__doc__


def test_the_pins_of_the_stereo_tests_still_hold():
    from vision import cv2_facade as f
    from vision.utils import feature, stereo
    bm = f.StereoBM_create()
    for name, value in (("SpeckleWindowSize", 50), ("SpeckleRange", 2), ("Disp12MaxDiff", 1)):
        with pytest.raises(f.error):
            getattr(bm, "set" + name)(value)
    img = np.zeros((20, 40), np.uint8)
    with pytest.raises(TypeError):
        stereo.stereo_depth(img, img, 500.0, 0.1, speckle_window_size=3)
    assert [p for p in inspect.signature(stereo.stereo_depth).parameters] == ["left", "right", "focal_px", "baseline_m", "matcher"]
    assert not hasattr(f, "StereoSGBM_create") and not hasattr(f, "StereoSGBM")
    for name in ("find_corners", "find_circles", "find_line_segments"):
        with pytest.raises(Exception):
            getattr(feature, name)(np.zeros((4, 4), np.uint8))
    with pytest.raises(Exception):
        f.fitEllipse(np.zeros((5, 1, 2), np.int32))
