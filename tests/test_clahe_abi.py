"""CPU suite for the surface of cv2.equalizeHist and CLAHE: the four C entries are exported by libvp.so and declared in include/vp.h
with the prototypes vision/_vp.py binds; every rejection the header lists answers with its code before any device work (no context
is needed to be refused, and a refused call writes nothing); the plan (csrc/vp_clahe_plan.h, run on the host under the address and
undefined-behaviour sanitizers by tests/native/clahe_plan_main.cpp) keeps shares, grids and LDS budgets within bounds; the facade
object's getters and setters round-trip and the facade raises on what is outside the path."""
import ctypes as C
import functools
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import clahe_restate as R
from abi_header import _header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vp_equalize_hist_u8", "vp_equalize_hist_dev", "vp_clahe_u8", "vp_clahe_dev"]


def test_clahe_symbols_are_exported_declared_and_bound_alike():
    from vision import _vp
    protos = _header_prototypes()
    lib = C.CDLL(_vp.LIB_PATH)
    for name in NEW:      # that each is bound as declared: test_abi.py::test_every_prototype_is_bound_as_declared
        assert hasattr(lib, name) and name in protos and name in _vp._SIGS, name
    built = open(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "build.py")).read()
    assert '"vp_clahe.hip"' in built, "vp_clahe.hip is not among VP_SOURCES"


def test_clahe_option_is_declared_and_bound():
    from vision import _vp
    txt = open(os.path.join(ROOT, "include", "vp.h")).read()
    m = re.search(r"VP_OPT_CLAHE_SPLIT\s*=\s*(\d+)", txt)
    assert m and int(m.group(1)) == _vp.OPT_CLAHE_SPLIT
    assert txt.count("VP_OPT_CLAHE_SPLIT") >= 2, "the option is documented with the others"


def _bound():
    from vision import _vp
    lib = C.CDLL(_vp.LIB_PATH)
    for name in NEW + ["vp_gaussian_blur_u8"]:
        res, args = _vp._SIGS[name]
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return _vp, lib


def test_every_rejection_answers_with_its_code_before_any_device_work_and_writes_nothing():
    """No context is passed: an accepted argument set then fails like the neighbouring entries do (VP_ERR_INVALID, as the blur), a
    rejected one has already answered with its own code.  The buffers are host arrays: nothing may touch them either way."""
    vp, lib = _bound()
    INV, UNS = vp.ERR_INVALID, vp.ERR_UNSUPPORTED
    w, h = 40, 30
    src = np.arange(w * h, dtype=np.uint32).astype(np.uint8).reshape(h, w)
    keep = src.copy()
    dst = np.full((2 * h, w), 77, np.uint8)
    s, d = src.ctypes.data, dst.ctypes.data
    blur = lib.vp_gaussian_blur_u8(None, s, w, h, 1, 3, 3, 0.0, 0.0, d)
    assert blur == INV
    nan, inf = float("nan"), float("inf")

    def clahe(form, src=s, stride=w, w=w, h=h, clip=2.0, tx=8, ty=8, dst=d):
        if form == "u8":
            return lib.vp_clahe_u8(None, src, w, h, clip, tx, ty, dst)
        return lib.vp_clahe_dev(None, src, stride, w, h, clip, tx, ty, dst)

    def eq(form, src=s, stride=w, w=w, h=h, dst=d):
        if form == "u8":
            return lib.vp_equalize_hist_u8(None, src, w, h, dst)
        return lib.vp_equalize_hist_dev(None, src, stride, w, h, dst)

    for form in ("u8", "dev"):
        assert clahe(form) == blur and eq(form) == blur, "accepted arguments without a context fail like the neighbours"
        for kw in (dict(src=None), dict(dst=None), dict(w=0), dict(h=0), dict(w=-3), dict(h=-1)):
            assert clahe(form, **kw) == INV and eq(form, **kw) == INV, (form, kw)
        for kw in (dict(tx=0), dict(ty=0), dict(tx=-1, ty=-1), dict(clip=nan), dict(clip=nan, tx=65)):
            assert clahe(form, **kw) == INV, (form, kw)
        for kw in (dict(tx=65), dict(ty=65), dict(tx=1000, ty=1000), dict(w=1 << 15, h=(1 << 13) + 1), dict(w=(1 << 28) + 1, h=1)):
            assert clahe(form, **kw) == UNS, (form, kw)
        for kw in (dict(w=1 << 15, h=(1 << 13) + 1), dict(w=(1 << 28) + 1, h=1)):
            assert eq(form, **kw) == UNS, (form, kw)
        # an extension that is not smaller than the dimension it reflects
        for kw in (dict(w=3, h=30, tx=8, ty=3), dict(w=40, h=2, tx=8, ty=4), dict(w=1, h=3, tx=1, ty=2), dict(w=4, h=4, tx=8, ty=8), dict(w=40, h=1, tx=8, ty=2)):
            assert not R.supported(kw["w"], kw["h"], 2.0, kw["tx"], kw["ty"])
            assert clahe(form, **kw) == UNS, (form, kw)
        for kw in (dict(w=5, h=30, tx=8, ty=3), dict(w=9, h=9, tx=8, ty=8), dict(w=1, h=1, tx=1, ty=1), dict(w=8, h=8, tx=8, ty=8)):
            assert R.supported(kw["w"], kw["h"], 2.0, kw["tx"], kw["ty"])
            assert clahe(form, **kw) == blur, (form, kw)
        # clip_limit * area / 256 from 2^31 on: 40 x 30 on (8, 8) is extended to 48 x 32, tiles of 6 x 4 = 24
        for clip in (2.0 ** 31 * 256 / 24, 1e300, inf):
            assert clahe(form, clip=clip) == UNS, (form, clip)
        for clip in (np.nextafter(2.0 ** 31 * 256 / 24, 0), -inf, -1.0, 0.0):
            assert clahe(form, clip=clip) == blur, (form, clip)
    # the device forms: a stride below the width, and dst overlapping src (dst starts inside the strided source)
    assert clahe("dev", stride=w - 1) == INV and eq("dev", stride=w - 1) == INV
    wide = np.zeros((h, 2 * w), np.uint8)
    p = wide.ctypes.data
    for off in (0, 1, w, (h - 1) * 2 * w + w - 1):
        assert clahe("dev", src=p, stride=2 * w, dst=p + off) == INV and eq("dev", src=p, stride=2 * w, dst=p + off) == INV, off
    assert clahe("dev", src=p, stride=2 * w, dst=p + (h - 1) * 2 * w + w) == blur      # just past the last source byte: accepted
    assert (dst == 77).all() and np.array_equal(src, keep) and not wide.any(), "a rejected call wrote to a buffer"


@functools.lru_cache(maxsize=None)
def _plan_output():
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the sanitizer build"
    import tempfile
    d = tempfile.mkdtemp(prefix="clahe_plan_")
    exe = os.path.join(d, "clahe_plan")
    try:
        build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                "-I" + os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc"), os.path.join(ROOT, "tests", "native", "clahe_plan_main.cpp"), "-o", exe],
                               capture_output=True, text=True, timeout=300)
        assert build.returncode == 0, build.stderr[-2000:]
        run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    return run.stdout.splitlines()


def test_plan_accepts_what_the_statement_accepts_and_keeps_shares_and_budgets_within_bounds():
    lines = _plan_output()
    max_tiles, max_px, hist_block, max_split, part_px, apply_block, apply_rows, budget = (int(v) for v in next(l for l in lines if l.startswith("tile ")).split()[1:])
    assert (max_tiles, max_px, hist_block, apply_block) == (64, 1 << 28, 256, 256) and budget <= 64 * 1024 and 1 <= max_split <= 64
    plans = [l for l in lines if l.startswith("plan ")]
    assert len(plans) > 10000
    accepted = 0
    for l in plans:
        a, b = l[5:].split("|")
        w, h, clip, tx, ty, opt = a.split()
        w, h, tx, ty, opt, clip = int(w), int(h), int(tx), int(ty), int(opt), float(clip)
        status, padded, ew, eh, tw, th, area, iclip, split, part_rows, in_lds, lds_bytes, hgx, hgy, agx = (int(v) for v in b.split())
        invalid = w <= 0 or h <= 0 or tx < 1 or ty < 1 or clip != clip
        if invalid:
            assert status == 1, l
            continue
        if not R.supported(w, h, clip, tx, ty):
            assert status == 2, l
            continue
        assert status == 0, l
        accepted += 1
        assert (ew, eh, tw, th) == R.geometry(w, h, tx, ty) and area == tw * th and padded == int((ew, eh) != (w, h)), l
        assert iclip == R.clip_count(clip, area), l
        assert 1 <= split <= min(max_split, th) and split * part_rows >= th and (split - 1) * part_rows < th, l      # every block has a row, every row a block
        want = opt                                       # blocks asked for: forced, or the fewest (a power of two) that leave a block part_px pixels at most
        if opt < 1:
            want = 1
            while want < max_split and -(-area // want) > part_px:
                want *= 2
        want = min(want, max_split, th)
        assert part_rows == -(-th // want) and split == -(-th // part_rows) and split <= want, l
        assert (hgx, hgy) == (tx * ty, split) and agx == -(-h // apply_rows), l
        assert in_lds == int(tx * ty * 256 <= budget) and lds_bytes == (tx * ty * 256 if in_lds else 0) and lds_bytes % 16 == 0, l
    assert accepted > 2000


def test_facade_object_round_trips_and_has_cv2s_names():
    from vision import cv2_facade as f
    assert list(inspect.signature(f.equalizeHist).parameters) == ["src", "dst"]
    assert list(inspect.signature(f.createCLAHE).parameters) == ["clipLimit", "tileGridSize"]
    p = inspect.signature(f.createCLAHE).parameters
    assert p["clipLimit"].default == 40.0 and p["tileGridSize"].default == (8, 8)
    c = f.createCLAHE()
    assert c.getClipLimit() == 40.0 and c.getTilesGridSize() == (8, 8)
    c = f.createCLAHE(2.0, (4, 3))
    assert c.getClipLimit() == 2.0 and c.getTilesGridSize() == (4, 3)
    c.setClipLimit(3)
    c.setTilesGridSize((16, 2))
    assert c.getClipLimit() == 3.0 and isinstance(c.getClipLimit(), float) and c.getTilesGridSize() == (16, 2)
    c = f.createCLAHE(clipLimit=1.5, tileGridSize=[2, 5])
    assert (c.getClipLimit(), c.getTilesGridSize()) == (1.5, (2, 5))
    assert c.collectGarbage() is None
    assert list(inspect.signature(c.apply).parameters) == ["src", "dst"]
    for bad in (lambda: c.setClipLimit(float("nan")), lambda: c.setClipLimit("x"), lambda: c.setTilesGridSize((0, 8)), lambda: c.setTilesGridSize((8,)),
                lambda: c.setTilesGridSize(8), lambda: f.createCLAHE(2.0, (8, -1))):
        with pytest.raises(f.error):
            bad()
    assert (c.getClipLimit(), c.getTilesGridSize()) == (1.5, (2, 5)), "a refused setter changed the object"
    from vision.utils import color
    assert list(inspect.signature(color.equalize_hist).parameters) == ["mat"]
    for fn in (color.clahe, color.clahe_bgr):
        q = inspect.signature(fn).parameters
        assert list(q) == ["mat", "clip_limit", "tile_grid"] and q["clip_limit"].default == 2.0 and q["tile_grid"].default == (8, 8)
        assert "addition" in fn.__doc__
    assert "addition" in color.equalize_hist.__doc__


def test_facade_raises_on_wrong_input_types_before_anything_is_launched():
    from vision import cv2_facade as f
    c = f.createCLAHE(2.0, (8, 8))
    bad = [np.zeros((6, 5, 3), np.uint8), np.zeros((6, 5, 2), np.uint8), np.zeros((6, 5), np.uint16), np.zeros((6, 5), np.float32), np.zeros((6, 5), np.int8),
           np.zeros((0, 5), np.uint8), np.zeros((6, 0), np.uint8), np.zeros((5,), np.uint8), np.zeros((2, 3, 4, 1), np.uint8)]
    for src in bad:
        with pytest.raises(f.error):
            c.apply(src)
        with pytest.raises(f.error):
            f.equalizeHist(src)
    with pytest.raises(f.error):
        f.createCLAHE(2.0, (65, 8)).apply(np.zeros((130, 16), np.uint8))
    from vision.utils import color
    g = np.zeros((6, 5), np.uint8)
    for call in (lambda: color.clahe(g, float("nan")), lambda: color.clahe(g, 2.0, (0, 8)), lambda: color.clahe(g, 2.0, 8), lambda: color.clahe_bgr(g, 2.0, (8, 0))):
        with pytest.raises(ValueError):
            call()
