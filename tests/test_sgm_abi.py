"""CPU suite for the surface of semi-global matching: the C entries are exported by libvp.so, declared in include/vp.h and bound alike;
the plan's candidate rectangle is the restatement's; every refusal is made from the arguments alone, names its reason and writes nothing
(no device needed: the checks come before the context is touched); the Python layer has the names, the defaults and the refusals; the
facade gains nothing."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import sgm_cases as SC
import stereo_restate as R
from abi_header import _header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vp_stereo_sgm_plan", "vp_stereo_sgm_u8", "vp_stereo_sgm_dev", "vp_stereo_sgm_host"]


def test_symbols_are_exported_declared_and_bound_alike():
    from vision import _vp
    protos = _header_prototypes()
    lib = C.CDLL(_vp.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name) and name in protos and name in _vp._SIGS, name
        assert protos[name][1] == list(_vp._SIGS[name][1]) and protos[name][0] == "int", name
    assert [len(protos[n][1]) for n in NEW] == [9, 15, 18, 17]
    built = open(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "build.py")).read()
    for src in ("vp_sgm.hip", "vp_api_sgm.hip"):
        assert f'"{src}"' in built, f"{src} is not among VP_SOURCES"
        assert os.path.exists(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc", src))
    assert os.path.exists(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc", "vp_sgm_plan.h"))
    header = open(os.path.join(ROOT, "include", "vp.h")).read()
    assert f"#define VP_SGM_GEOMETRY {SC.GEOMETRY}\n" in header and "4294967296" in header


def test_plan_rectangle_is_the_statements():
    from vision.utils import stereo
    for h in (1, 4, 9, 40):
        for bs in range(1, 10, 2):
            for n in (16, 32):
                for m in (-3, 0, 4):
                    for w in range(1, 81):
                        want = R.valid_rect(w, h, n, bs, m)
                        assert SC.lib_plan(w, h, n, bs, m)["rect"] == want, (w, h, n, bs, m)
                    assert stereo.valid_rect_sgm(60, h, n, bs, m) == R.valid_rect(60, h, n, bs, m)
    assert stereo.valid_rect_sgm(640, 480) == R.valid_rect(640, 480, 64, 5, 0) == (65, 2, 573, 476)
    assert stereo.valid_rect_sgm(19, 5, 16, 5) == (0, 0, 0, 0)


def test_plan_geometry_and_workspace():
    for n in range(16, 257, 16):
        for bs in (1, 9):
            for w, h in ((20, 5), (640, 480), (1280, 720), (1920, 1080)):
                for paths in (4, 8):
                    p = SC.lib_plan(w, h, n, bs, 0, paths)
                    x, y, cw, ch = p["rect"]
                    cost, path, sel = p["cost"], p["path"], p["select"]
                    assert cost["threads"] == 256 and 0 < cost["lds_bytes"] <= 65536 and cost["grid"] == (-(-cw // cost["strip_cols"]), ch)
                    assert path["threads"] == 64 and path["group"] in (16, 32, 64) and path["per_lane"] in (1, 2, 4) and path["group"] * path["per_lane"] >= n
                    assert path["lines_per_block"] * path["group"] == 64
                    assert path["grid_d"] == (0 if paths == 4 or not cw else -(-(cw + ch - 1) // path["lines_per_block"]))
                    assert sel["threads"] == 256 and sel["px_per_block"] * path["group"] == 256 and sel["grid"] == -(-(cw * ch) // sel["px_per_block"])
                    assert p["ws_bytes"] >= 2 * w * h + 4 * cw * ch * n and p["ws_bytes"] <= 2 * (w + 3) * h + 4 * cw * ch * n + 4 * 256
    assert SC.lib_plan(19, 5, 16, 5, 0)["cost"]["grid"] == (0, 0)
    # below the cap S lies more than 2^31 bytes from the workspace's start and a volume holds close to 2^30 entries: the indices are size_t
    big = SC.lib_plan(4096, 1090, 256, 5, 0)
    assert big["ws_bytes"] > 2 ** 31 and big["rect"][2] * big["rect"][3] * 256 > 2 ** 30 - 2 ** 24


def test_workspace_cap_is_4_gib():
    from vision import _vp
    lib = _vp.lib()
    rect, geom, ws = (C.c_int32 * 4)(*[7] * 4), (C.c_int32 * SC.GEOMETRY)(*[7] * SC.GEOMETRY), C.c_size_t(7)
    assert lib.vp_stereo_sgm_plan(4096, 4096, 256, 5, 0, 8, rect, C.byref(ws), geom) == _vp.ERR_INVALID
    assert "4294967296" in lib.vp_last_error(None).decode() and list(rect) == [7] * 4 and list(geom) == [7] * SC.GEOMETRY and ws.value == 7
    # the largest admitted and the smallest refused height at 4096 columns and 256 disparities
    fits = [h for h in range(1000, 1200) if lib.vp_stereo_sgm_plan(4096, h, 256, 5, 0, 8, rect, C.byref(ws), geom) == 0]
    assert fits and fits[-1] < 1199 and fits == list(range(1000, fits[-1] + 1))
    assert SC.lib_plan(4096, fits[-1], 256, 5, 0)["ws_bytes"] <= 2 ** 32


GOOD = dict(w=40, h=12, n=16, bs=5, m=0, c=31, p1=8, p2=32, u=10, d=1, paths=8)


def _calls(lib, left, right, disp, ls, rs, ds, a):
    """the three matcher entries on one argument set (ctx NULL: a call that passed its checks would stop at the context)"""
    tail = (a["w"], a["h"], a["n"], a["bs"], a["m"], a["c"], a["p1"], a["p2"], a["u"], a["d"], a["paths"])
    yield "host", lambda: lib.vp_stereo_sgm_host(left, ls, right, rs, *tail, disp, ds)
    yield "dev", lambda: lib.vp_stereo_sgm_dev(None, left, ls, right, rs, *tail, disp, ds)
    if ls == rs == a["w"] and ds == 2 * a["w"]:
        yield "u8", lambda: lib.vp_stereo_sgm_u8(None, left, right, *tail, disp)


P2_MAX = SC.largest_p2(8, 31, 5)
REFUSALS = [
    ("pointer", dict(left=None)), ("pointer", dict(right=None)), ("pointer", dict(disp=None)),
    ("width", dict(w=0)), ("4096", dict(w=4097)), ("height", dict(h=0)), ("4096", dict(h=4097)),
    ("stride", dict(ls=39)), ("stride", dict(rs=39)), ("stride", dict(ds=79)), ("element size", dict(ds=81)),
    ("num_disparities", dict(n=0)), ("num_disparities", dict(n=24)), ("num_disparities", dict(n=272)),
    ("block_size", dict(bs=-1)), ("block_size", dict(bs=0)), ("block_size", dict(bs=4)), ("block_size", dict(bs=11)),
    ("min_disparity", dict(m=-129)), ("min_disparity", dict(m=129)),
    ("pre_filter_cap", dict(c=0)), ("pre_filter_cap", dict(c=64)),
    ("negative", dict(p1=-1)), ("negative", dict(p1=-1, p2=-1)), ("p1 must not exceed p2", dict(p1=33)),
    ("uniqueness_ratio", dict(u=-1)), ("uniqueness_ratio", dict(u=101)),
    ("disp12_max_diff", dict(d=-2)), ("disp12_max_diff", dict(d=256)),
    ("paths", dict(paths=3)), ("paths", dict(paths=5)), ("paths", dict(paths=9)), ("paths", dict(paths=16)),
    ("65535", dict(p2=P2_MAX + 1)), ("65535", dict(p2=2 ** 31 - 1)),
    ("aligned", dict(odd=True)), ("overlaps", dict(alias="left")), ("overlaps", dict(alias="right")),
]


@pytest.mark.parametrize("word,change", REFUSALS, ids=[f"{w.split()[0]}-{'-'.join(f'{k}{v}' for k, v in c.items())}" for w, c in REFUSALS])
def test_refusals_name_the_reason_and_write_nothing(word, change):
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
    if "odd" in change:
        ptrs["disp"] += 1
    ls, rs, ds = change.get("ls", a["w"]), change.get("rs", a["w"]), change.get("ds", 2 * a["w"])
    ran = 0
    for form, call in _calls(lib, ptrs["left"], ptrs["right"], ptrs["disp"], ls, rs, ds, a):
        assert call() == _vp.ERR_INVALID, form
        assert word in lib.vp_last_error(None).decode(), (form, lib.vp_last_error(None))
        ran += 1
    assert ran >= 2 and np.all(buf == 0x5A)
    if set(change) <= {"w", "h", "n", "bs", "m", "paths"}:       # the plan refuses the same geometry
        rect, geom, ws = (C.c_int32 * 4)(*[7] * 4), (C.c_int32 * SC.GEOMETRY)(*[7] * SC.GEOMETRY), C.c_size_t(7)
        assert lib.vp_stereo_sgm_plan(a["w"], a["h"], a["n"], a["bs"], a["m"], a["paths"], rect, C.byref(ws), geom) == _vp.ERR_INVALID
        assert word in lib.vp_last_error(None).decode() and list(rect) == [7] * 4 and list(geom) == [7] * SC.GEOMETRY and ws.value == 7


def test_the_bounds_themselves_are_admitted():
    """every range at both ends, and the 16-bit bound at the bound: the host routine runs"""
    left, right = SC.shifted_pair(12, 300, 3, 1)
    for change in (dict(num_disparities=16), dict(num_disparities=256), dict(block_size=1), dict(block_size=9), dict(min_disparity=-128), dict(min_disparity=128),
                   dict(pre_filter_cap=1), dict(pre_filter_cap=63, p1=50, p2=100), dict(p1=0, p2=0), dict(uniqueness_ratio=0), dict(uniqueness_ratio=100),
                   dict(disp12_max_diff=-1), dict(disp12_max_diff=255), dict(paths=4), dict(p1=P2_MAX, p2=P2_MAX, pre_filter_cap=31, block_size=5, paths=8)):
        out = SC.host_disparity(left, right, **{"num_disparities": 16, **change})
        assert out.shape == left.shape


def test_an_image_without_candidates_is_no_error():
    left, right = SC.shifted_pair(5, 19, 1)
    assert np.all(SC.host_disparity(left, right, num_disparities=16, block_size=5) == -16)


def test_python_names_signatures_and_refusals():
    from vision.utils import stereo
    sig = lambda fn: [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    matcher = [("num_disparities", 64), ("block_size", 5), ("min_disparity", 0), ("pre_filter_cap", 31), ("p1", None), ("p2", None), ("uniqueness_ratio", 10),
               ("disp12_max_diff", 1), ("paths", 8)]
    assert sig(stereo.disparity_sgm) == [("left", E), ("right", E)] + matcher
    assert sig(stereo.valid_rect_sgm) == [("w", E), ("h", E)] + matcher[:3]
    assert [n for n, _ in sig(stereo.stereo_depth_sgm)] == ["left", "right", "focal_px", "baseline_m", "matcher"]
    assert sig(stereo.stereo_planes_sgm) == [("left", E), ("right", E), ("focal_px", E), ("baseline_m", E), ("cx", None), ("cy", None), ("speckle_window_size", 100),
                                             ("speckle_range", 2), ("max_jump_m", None), ("matcher", E)]
    # the block matcher's surface is as it was
    assert [n for n, _ in sig(stereo.stereo_depth)] == ["left", "right", "focal_px", "baseline_m", "matcher"]
    assert sig(stereo.stereo_planes)[4:] == sig(stereo.stereo_planes_sgm)[4:]
    # p1 = None and p2 = None are 8 and 32 block_size^2
    assert stereo._matcher_sgm() == (64, 5, 0, 31, 200, 800, 10, 1, 8)
    assert stereo._matcher_sgm(block_size=3)[4:6] == (72, 288) and stereo._matcher_sgm(block_size=3, p1=5)[4:6] == (5, 288)
    assert stereo._matcher_sgm(p1=P2_MAX, p2=P2_MAX)[5] == P2_MAX
    assert "nothing here measured" in stereo.disparity_sgm.__doc__
    img = np.zeros((20, 40), np.uint8)
    for bad in (dict(num_disparities=0), dict(num_disparities=24), dict(num_disparities=272), dict(block_size=-1), dict(block_size=4), dict(block_size=11),
                dict(min_disparity=-129), dict(min_disparity=129), dict(pre_filter_cap=0), dict(pre_filter_cap=64), dict(p1=-1), dict(p2=-1), dict(p1=33, p2=32),
                dict(p1=900), dict(uniqueness_ratio=-1), dict(uniqueness_ratio=101), dict(disp12_max_diff=-2), dict(disp12_max_diff=256), dict(paths=3), dict(paths=6),
                dict(paths=9), dict(p2=P2_MAX + 1), dict(block_size=9, pre_filter_cap=63)):      # 8 * (2 * 63 * 81 + 32 * 81) passes the 16-bit bound
        for call in (lambda: stereo.disparity_sgm(img, img, **bad), lambda: stereo.stereo_depth_sgm(img, img, 500.0, 0.1, **bad),
                     lambda: stereo.stereo_planes_sgm(img, img, 500.0, 0.1, **bad)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError, match="65535"):
        stereo.disparity_sgm(img, img, p2=P2_MAX + 1)
    for bad in (dict(num_disparities=64.0), dict(block_size="5"), dict(p1=8.0), dict(p2=True), dict(paths=8.0), dict(disp12_max_diff=None), dict(uniqueness_ratio=1.5)):
        with pytest.raises(TypeError):
            stereo.disparity_sgm(img, img, **bad)
    with pytest.raises(ValueError):
        stereo.disparity_sgm(img, img[:, :30])                               # images of different sizes
    with pytest.raises(TypeError):
        stereo.disparity_sgm(img.astype(np.float32), img)                    # float images
    with pytest.raises(TypeError):
        stereo.stereo_depth_sgm(img, img, 500.0, 0.1, texture_threshold=3)    # the block matcher's key
    with pytest.raises(TypeError):
        stereo.stereo_planes_sgm(img, img, 500.0, 0.1, speckle=3)
    with pytest.raises(TypeError):
        stereo.stereo_depth(img, img, 500.0, 0.1, p1=3)                      # and the block matcher refuses this one's
    with pytest.raises(ValueError):
        stereo.valid_rect_sgm(4097, 10)


def test_the_facade_gains_nothing():
    from vision import cv2_facade as f
    assert not [n for n in dir(f) if n.startswith("StereoSGBM")]
    assert not [n for n in dir(f.install()) if n.startswith("StereoSGBM")]
    bm = f.StereoBM_create(32, 9)
    with pytest.raises(f.error):
        bm.setDisp12MaxDiff(1)
