"""CPU suite: the C-ABI library loads and exports every symbol include/vp.h declares; host-only entry
points (structuring elements, tables, error paths) behave; no compute call is made without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from abi_header import _header_prototypes, _header_text, header_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b([a-z_0-9]+)\s*\(", " ".join(l for l in txt.splitlines() if not l.strip().startswith("#")))))


def test_libvp_exports_every_declared_symbol():
    from vision import _vp
    names = [n for n in _declared("vp.h") if n.startswith("vp_")]
    assert len(names) >= 25
    lib = C.CDLL(_vp.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"libvp.so does not export {n}"
    assert set(_vp.exported_symbols()) == set(names), set(_vp.exported_symbols()) ^ set(names)


def test_every_prototype_is_bound_as_declared():
    """Return type and argument list of every prototype of include/vp.h against vision/_vp.py's _SIGS, and every VP_OPT_* against its
    OPT_*: the one place that says "declared and bound alike" (the *_abi files keep what is their family's own)."""
    from vision import _vp
    protos, header = _header_prototypes(), _header_text()
    assert set(protos) == set(n for n in _declared("vp.h") if n.startswith("vp_")), "a declaration the prototype parser does not read"
    assert set(protos) == set(_vp._SIGS), set(protos) ^ set(_vp._SIGS)
    returns = {"int": C.c_int, "const char*": C.c_char_p, "void*": C.c_void_p, "vp_ctx*": C.c_void_p, "vp_feeder*": C.c_void_p,
               "unsigned int": C.c_uint, "uint64_t": C.c_uint64}
    for name, (ret, types) in protos.items():
        res, args = _vp._SIGS[name]
        assert ret in returns and res is returns[ret], (name, ret, res)
        # a typed pointer or a char* binds a pointer argument as well as void* does
        bound = [C.c_void_p if a is C.c_char_p or (isinstance(a, type) and issubclass(a, C._Pointer)) else a for a in args]
        assert bound == types, (name, bound, types)
        if re.search(name + r"\s*\(\s*(const\s+)?vp_ctx\s*\*", header):
            assert args[0] is C.c_void_p, (name, "the context is bound as void*")
    options = header_options()
    assert len(options) == 11 and sorted(options.values()) == list(range(1, 12))
    assert options == {n[4:]: getattr(_vp, n) for n in dir(_vp) if n.startswith("OPT_")}


def test_host_only_entry_points(oracle):
    from vision import _vp
    L = _vp.lib()
    assert L.vp_version() >= 100
    assert L.vp_strerror(0) == b"ok" and L.vp_strerror(-2) == b"HIP runtime error"
    g, c, s, hd, lc = _vp.get_tables()
    og, oc, os_, oh, olc = oracle.tables()
    assert np.array_equal(g, og) and np.array_equal(c, oc) and np.array_equal(s, os_) and np.array_equal(hd, oh)
    assert lc.tolist() == olc.tolist()
    from vision.utils import transform as T
    for k in (1, 3, 5, 7, 15, 101):
        assert np.array_equal(T.elliptic_kernel(k), oracle.structuring_element(oracle.MORPH_ELLIPSE, k, k))
    assert T.rect_kernel(3, 2).shape == (2, 3)
    with pytest.raises(ValueError):
        T.elliptic_kernel(2)
    with pytest.raises(ValueError):
        T.rect_kernel(-1)
    out = np.zeros(4, np.uint8)
    assert L.vp_structuring_element(7, 2, 2, out.ctypes.data_as(C.c_void_p)) == -1


def test_no_cpu_fallback():
    """Without a GPU every operator must fail loudly — the product never routes through the oracle."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu suite")
    from vision import _vp
    from vision.utils import color
    with pytest.raises(_vp.VpError):
        color.bgr_to_lab(np.zeros((4, 4, 3), np.uint8))
    assert _vp.lib().vp_create(0) is None


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "cuauv-vision-pipeline_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h")):
                txt = open(os.path.join(dp, f), errors="ignore").read()
                assert "oracle" not in txt.replace("the oracle", "").replace("against the oracle", "") or f in ("_vp.py",) or "oracle/" not in txt, f


def test_polygon_helpers():
    from vision.utils import feature
    sq = np.array([[[2, 2]], [[2, 6]], [[6, 6]], [[6, 2]]], np.int32)
    assert feature.contour_area(sq) == 16.0
    assert feature.contour_centroid(sq) == (4, 4)
    assert feature.contour_centroid(np.array([[[3, 3]]], np.int32)) == (0, 0)  # degenerate: m00 clamped (utils/feature.py:251)
    assert feature.contour_perimeter(sq) == 16.0 and feature.contour_perimeter(sq, closed=False) == 12.0
    big = np.array([[[0, 0]], [[0, 50]], [[1, 100]], [[100, 100]], [[100, 0]]], np.int32)
    assert feature.contour_approx(big, epsilon=2.0).reshape(-1, 2).tolist() == [[0, 0], [1, 100], [100, 100], [100, 0]]
    (cx, cy), (w, h), ang = feature.min_enclosing_rect(sq)
    assert (cx, cy) == (4.0, 4.0) and sorted((w, h)) == [4.0, 4.0] and ang == 90.0
    with pytest.raises(NotImplementedError):
        feature.find_circles(sq)


def test_color_balance_library_exports_reference_entry():
    """libauv-color-balance.so (modules/color_balance.py:12) exports process_frame with the reference's argument list
    (utils/color_correction/color_balance.hpp:9-14); no compute call here."""
    names = _declared("color_balance_c.h")
    assert "process_frame" in names
    lib = C.CDLL(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "lib", "libauv-color-balance.so"))
    for n in names:
        assert hasattr(lib, n), n
    import torch
    if not torch.cuda.is_available():
        arr = np.zeros((4, 4, 3), np.uint8)
        lib.process_frame.restype = C.c_int
        rc = lib.process_frame(arr.ctypes.data_as(C.c_void_p), C.c_size_t(4), C.c_size_t(4), C.c_size_t(3), True, False, True, False, True, False, 1, 1)
        assert rc == -2          # VP_ERR_HIP: no device, no CPU path
        assert lib.process_frame(arr.ctypes.data_as(C.c_void_p), C.c_size_t(4), C.c_size_t(4), C.c_size_t(4), True, False, True, False, True, False, 1, 1) == -1


def test_facade_positional_order_is_cv2s():
    """A module written against the real cv2 may pass dst / anchor / iterations positionally: the facade takes them in cv2's order
    (cv2.erode(src, kernel, dst, anchor, iterations, borderType, borderValue), ...)."""
    import inspect
    from vision import cv2_facade as f
    want = {"erode": ["src", "kernel", "dst", "anchor", "iterations", "borderType", "borderValue"],
            "dilate": ["src", "kernel", "dst", "anchor", "iterations", "borderType", "borderValue"],
            "morphologyEx": ["src", "op", "kernel", "dst", "anchor", "iterations", "borderType", "borderValue"],
            "GaussianBlur": ["src", "ksize", "sigmaX", "dst", "sigmaY", "borderType"],
            "warpAffine": ["src", "M", "dsize", "dst", "flags", "borderMode", "borderValue"],
            "resize": ["src", "dsize", "dst", "fx", "fy", "interpolation"]}
    for name, params in want.items():
        assert list(inspect.signature(getattr(f, name)).parameters) == params, name
