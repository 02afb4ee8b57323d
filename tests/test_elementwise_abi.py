"""CPU suite for the element-wise operators: the six entries of csrc/vp_elementwise.hip are exported by libvp.so, declared in
include/vp.h and bound by vision/_vp.py with the same argument types; the cv2 stand-in has the new names in cv2's parameter order,
rejects what cv2 rejects, and its numpy paths (numpy in, numpy out) make the float64 statement of image-with-scalar arithmetic."""
import ctypes as C
import inspect

import numpy as np
import pytest

from abi_header import _header_prototypes

NEW = ["vp_bitwise_u8_dev", "vp_arith_u8_dev", "vp_lut_u8_dev", "vp_split_u8_dev", "vp_merge_u8_dev", "vp_count_nonzero_u8_dev"]


def test_new_symbols_are_exported_declared_and_bound_alike():
    from vision import _vp
    protos = _header_prototypes()
    lib = C.CDLL(_vp.LIB_PATH)
    for name in NEW:      # that each is bound as declared: test_abi.py::test_every_prototype_is_bound_as_declared
        assert hasattr(lib, name) and name in protos and name in _vp._SIGS, name
    import re
    import os
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vp.h")).read()
    for name, value in (("VP_BITWISE_AND", _vp.BITWISE_AND), ("VP_BITWISE_OR", _vp.BITWISE_OR), ("VP_BITWISE_XOR", _vp.BITWISE_XOR),
                        ("VP_BITWISE_NOT", _vp.BITWISE_NOT), ("VP_ARITH_ADD", _vp.ARITH_ADD), ("VP_ARITH_SUB", _vp.ARITH_SUB),
                        ("VP_ARITH_ABSDIFF", _vp.ARITH_ABSDIFF)):
        m = re.search(name + r"\s*=\s*(\d+)", txt)
        assert m and int(m.group(1)) == value, name


def test_facade_names_have_cv2s_parameter_order():
    from vision import cv2_facade as f
    order = {"bitwise_and": ["src1", "src2", "dst", "mask"], "bitwise_or": ["src1", "src2", "dst", "mask"],
             "bitwise_xor": ["src1", "src2", "dst", "mask"], "bitwise_not": ["src", "dst", "mask"], "add": ["src1", "src2", "dst"],
             "subtract": ["src1", "src2", "dst"], "absdiff": ["src1", "src2", "dst"], "LUT": ["src", "lut"], "split": ["m"], "merge": ["mv"],
             "extractChannel": ["src", "coi"], "countNonZero": ["src"]}
    for name, params in order.items():
        assert hasattr(f, name), f"cv2_facade has no {name}"
        assert list(inspect.signature(getattr(f, name)).parameters)[:len(params)] == params, name


def test_facade_rejects_what_cv2_rejects():
    from vision import cv2_facade as f
    a = np.zeros((6, 5, 3), np.uint8)
    g = np.zeros((6, 5), np.uint8)
    flt = np.zeros((6, 5, 3), np.float32)
    empty = np.zeros((0, 5, 3), np.uint8)
    for fn in (f.bitwise_and, f.bitwise_or, f.bitwise_xor, f.add, f.subtract, f.absdiff):
        for x, y in ((a, np.zeros((6, 4, 3), np.uint8)), (a, g), (a, np.zeros((5, 6, 3), np.uint8)),      # size / channel mismatch
                     (empty, empty), (flt, flt), (a, flt), (flt, a)):
            with pytest.raises(f.error):
                fn(x, y)
    for x in (empty, flt):
        with pytest.raises(f.error):
            f.bitwise_not(x)
        with pytest.raises(f.error):
            f.LUT(x, np.arange(256, dtype=np.uint8))
        with pytest.raises(f.error):
            f.add(x, 3)
    for fn in (f.bitwise_and, f.bitwise_or, f.bitwise_xor):
        with pytest.raises(f.error):
            fn(a, a, np.empty_like(a), g)                                  # dst and mask together: outside the accelerated path
        with pytest.raises(f.error):
            fn(a, a, mask=np.zeros((6, 4), np.uint8))                      # mask of another size
        with pytest.raises(f.error):
            fn(a, a, mask=np.zeros((6, 5), np.float32))                    # mask of another type
    with pytest.raises(f.error):
        f.bitwise_not(a, np.empty_like(a), g)
    for bad_lut in (np.arange(255, dtype=np.uint8), np.arange(256, dtype=np.int32), np.zeros((256, 2), np.uint8)):
        with pytest.raises(f.error):
            f.LUT(a, bad_lut)
    with pytest.raises(f.error):
        f.countNonZero(a)                                                  # single channel only, as in cv2
    with pytest.raises(f.error):
        f.extractChannel(a, 3)
    with pytest.raises(f.error):
        f.add(a, (1, 2))                                                   # fewer values than channels


SCALARS = [-300, -20, -0.5, 0, 0.5, 1.5, 10, 255, 300]


def _sat(acc):
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def test_numpy_scalar_arithmetic_is_the_float64_statement():
    from vision import cv2_facade as f
    rng = np.random.default_rng(5)
    bgr = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    bgr.ravel()[:256] = np.arange(256)                                     # every byte value occurs
    gray = np.ascontiguousarray(bgr[:, :, 0])
    for img in (bgr, gray):
        a = img.astype(np.float64)
        for s in SCALARS:
            for got, exp in ((f.add(img, s), _sat(a + float(s))), (f.add(s, img), _sat(a + float(s))),
                             (f.subtract(img, s), _sat(a - float(s))), (f.subtract(s, img), _sat(float(s) - a)),
                             (f.absdiff(img, s), _sat(np.abs(a - float(s)))), (f.absdiff(s, img), _sat(np.abs(a - float(s))))):
                assert type(got) is np.ndarray and got.dtype == np.uint8 and np.array_equal(got, exp), s
    t = (1, -2, 300)
    a = bgr.astype(np.float64)
    tv = np.array(t, np.float64)
    assert np.array_equal(f.add(t, bgr), _sat(a + tv)) and np.array_equal(f.add(bgr, t), _sat(a + tv))
    assert np.array_equal(f.subtract(bgr, t), _sat(a - tv)) and np.array_equal(f.subtract(t, bgr), _sat(tv - a))
    assert np.array_equal(f.absdiff(bgr, t), _sat(np.abs(a - tv)))
    assert f.add(10, np.array([[250, 3]], np.uint8)).tolist() == [[255, 13]]


def test_numpy_images_give_numpy_results():
    from vision import cv2_facade as f
    rng = np.random.default_rng(6)
    a = rng.integers(0, 256, (7, 13, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (7, 13, 3), dtype=np.uint8)
    m = rng.choice(np.array([0, 7, 255], np.uint8), (7, 13))
    keep = (m != 0)[:, :, None]
    ai, bi = a.astype(np.int32), b.astype(np.int32)
    cases = [(f.bitwise_and(a, b), a & b), (f.bitwise_or(a, b), a | b), (f.bitwise_xor(a, b), a ^ b), (f.bitwise_not(a), ~a),
             (f.bitwise_and(a, a, mask=m), np.where(keep, a, 0)), (f.bitwise_not(a, mask=m), np.where(keep, ~a, 0)),
             (f.bitwise_or(a, 0xF0), a | 0xF0),
             (f.add(a, b), np.clip(ai + bi, 0, 255)), (f.subtract(a, b), np.clip(ai - bi, 0, 255)), (f.absdiff(a, b), np.abs(ai - bi)),
             (f.LUT(a, np.arange(256, dtype=np.uint8)[::-1].copy()), 255 - a), (f.extractChannel(a, 2), a[:, :, 2]),
             (f.merge(f.split(a)), a)]
    lut3 = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    cases.append((f.LUT(a, lut3), np.stack([lut3[:, c][a[:, :, c]] for c in range(3)], axis=2)))
    cases.append((f.LUT(a, lut3.reshape(1, 256, 3)), np.stack([lut3[:, c][a[:, :, c]] for c in range(3)], axis=2)))
    for got, exp in cases:
        assert type(got) is np.ndarray and got.dtype == np.uint8 and np.array_equal(got, exp)
    assert all(type(p) is np.ndarray for p in f.split(a)) and len(f.split(a[:, :, 0])) == 1
    assert f.countNonZero(m) == int(np.count_nonzero(m)) and f.countNonZero(np.zeros((3, 3), np.uint8)) == 0
    dst = np.empty_like(a)
    assert f.add(a, b, dst) is dst and np.array_equal(dst, np.clip(ai + bi, 0, 255))
