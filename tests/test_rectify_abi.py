"""CPU suite for stereo rectification and 3-D reprojection: the library's host statements (vp_rectify_pair_host, vp_reproject_to_3d_host)
byte for byte and bit for bit against tests/rectify_restate.py over tests/rectify_cases.py; every refusal of the entries, without a
context; the sources, the plan and the facade names.  No compute call needs a device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import rectify_cases as RC
import rectify_restate as R
from abi_header import header_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc")
INVALID = -1
INT_MIN = -2 ** 31


def _p(a):
    return None if a is None else a.ctypes.data


def host_rectify(left, right, tl, tr, keep="both", pads=(0, 0, 0, 0)):
    """vp_rectify_pair_host on images with padded strides -> (rc, grey left, grey right, colour left | None, colour right | None)"""
    from vision import _vp
    cn = 1 if left.ndim == 2 else left.shape[2]
    h, w = left.shape[:2]
    oh, ow = tl[1].shape
    spad, gpad, cpad, _ = pads
    src = []
    for img in (left, right):
        buf = np.full((h, w * cn + spad), 0x5A, np.uint8)
        buf[:, :w * cn] = img.reshape(h, w * cn)
        src.append(buf)
    grey = [np.full((oh, ow + gpad), 0xA5, np.uint8) for _ in range(2)]
    col = [np.full((oh, ow * cn + cpad), 0xA5, np.uint8) if keep == "both" or (keep == "left" and e == 0) else None for e in range(2)]
    rc = _vp.lib().vp_rectify_pair_host(_p(src[0]), w * cn + spad, _p(src[1]), w * cn + spad, w, h, cn, _p(tl[0]), _p(tl[1]), _p(tr[0]), _p(tr[1]), ow, oh,
                                        _p(grey[0]), ow + gpad, _p(grey[1]), ow + gpad, _p(col[0]), ow * cn + cpad, _p(col[1]), ow * cn + cpad)
    for g in grey:
        assert np.all(g[:, ow:] == 0xA5), "the padding of a grey result was written"
    for c in col:
        assert c is None or np.all(c[:, ow * cn:] == 0xA5), "the padding of a colour result was written"
    shape = (oh, ow) if cn == 1 else (oh, ow, cn)
    return (rc, grey[0][:, :ow], grey[1][:, :ow]) + tuple(None if c is None else c[:, :ow * cn].reshape(shape) for c in col)


def test_sources_plan_and_options():
    from vision import _vp
    built = open(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "build.py")).read()
    for src in ("vp_rectify.hip", "vp_api_rectify.hip"):
        assert f'"{src}"' in built, f"{src} is not among VP_SOURCES"
        assert os.path.exists(os.path.join(CSRC, src))
    assert len(header_options()) == 11, "rectification adds no option"
    header = open(os.path.join(ROOT, "include", "vp.h")).read()
    assert "VP_DISP_I16 = 0, VP_DISP_F32 = 1" in header
    from vision.utils import stereo
    assert (stereo.DISP_I16, stereo.DISP_F32) == (0, 1)
    text = open(os.path.join(CSRC, "vp_rectify_plan.h")).read()
    num = lambda n: int(re.search(r"#define " + n + r" (\d+)", text).group(1))
    p = RC.plan(61, 37, 3, 257, 5)
    assert (p["tile_w"], p["tile_h"], p["ppt"]) == (num("RP_TW"), num("RP_TH"), num("RP_PPT")) and p["tile_w"] == 64 * p["ppt"]
    assert p["grid"] == (2, 2, 2), "two tiles across, two down, the eye is the third grid dimension"
    kernel = open(os.path.join(CSRC, "vp_rectify.hip")).read()
    assert '#include "vp_rectify_plan.h"' in kernel and "blockIdx.z" in kernel and "vp_rectify_sample" in kernel and "vp_reproject_i16" in kernel
    g = (C.c_int32 * 6)()
    for bad in ((0, 4, 3, 4, 4), (4, 4, 2, 4, 4), (4, 4, 5, 4, 4), (4097, 4, 3, 4, 4), (4, 4, 3, 4, 4097), (4, 4, 3, 0, 4)):
        assert _vp.lib().vp_rectify_pair_plan(*bad, g) == INVALID, bad
    assert _vp.lib().vp_rectify_pair_plan(4, 4, 3, 4, 4, None) == INVALID


CASES = RC.cases(256, 4)


def test_case_tile_is_the_plans():
    p = RC.plan()
    assert (p["tile_w"], p["tile_h"]) == (256, 4), "tests/test_rectify_abi.py builds its cases for this tile"


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_host_rectify_is_the_statement(case):
    left, right, tl, tr = RC.inputs(case)
    want = RC.expected(case)
    if case["table"] == "outside":
        assert not want[0].any() and not want[2].any(), "every tap lies outside: the result is the border value"
    for pads in ((0, 0, 0, 0), (3, 5, 7, 0)):
        rc, gl, gr, cl, cr = host_rectify(left, right, tl, tr, case["keep"], pads)
        assert rc == 0
        assert np.array_equal(gl, want[0]) and np.array_equal(gr, want[1]), f"{int((gl != want[0]).sum() + (gr != want[1]).sum())} grey pixels differ"
        assert (cl is None) == (case["keep"] == "none") and (cr is None) == (case["keep"] != "both")
        assert cl is None or np.array_equal(cl, want[2])
        assert cr is None or np.array_equal(cr, want[3])


def test_a_tap_beside_the_eye_is_the_border_not_the_neighbour():
    """the left half of a side-by-side frame, black, beside a white right half: a left tap at column w - 1 + fraction blends with 0"""
    from vision import _vp
    w, h = 6, 4
    frame = np.zeros((h, 2 * w, 3), np.uint8)
    frame[:, w:] = 255
    xy = np.zeros((h, w, 2), np.int16)
    xy[..., 0], xy[..., 1] = w - 1, np.arange(h)[:, None]
    frac = np.full((h, w), 7 * 32 + 19, np.uint16)
    ident = RC.table("identity", w, h, w, h, 0)
    grey = [np.full((h, w), 9, np.uint8) for _ in range(2)]
    rc = _vp.lib().vp_rectify_pair_host(frame.ctypes.data, 6 * w, frame.ctypes.data + 3 * w, 6 * w, w, h, 3, _p(xy), _p(frac), _p(ident[0]), _p(ident[1]), w, h,
                                        _p(grey[0]), w, _p(grey[1]), w, None, 0, None, 0)
    assert rc == 0 and not grey[0].any() and np.all(grey[1] == 255)
    assert np.array_equal(grey[0], R.rectify_eye(frame[:, :w], xy, frac)[0])


REPROJECT = RC.reproject_cases()


@pytest.mark.parametrize("case", REPROJECT, ids=[c["id"] for c in REPROJECT])
def test_host_reproject_is_the_statement(case):
    """products and sums are written without fma on both sides: the library is built with contraction off and the shared formula
    (vp_rectify_plan.h) says so again by pragma; numpy never fuses."""
    from vision import _vp
    disp, q = case["disp"], np.ascontiguousarray(case["Q"])
    h, w = disp.shape
    want = R.reproject(disp, q, case["invalid"])
    kind = 0 if disp.dtype == np.int16 else 1
    inv = INT_MIN if case["invalid"] is None else case["invalid"]
    for dpad, xpad in ((0, 0), (3, 5)):
        buf = np.zeros((h, w + dpad), disp.dtype)
        buf[:, :w] = disp
        out = np.full((h, 3 * w + xpad), 777.0, np.float32)
        rc = _vp.lib().vp_reproject_to_3d_host(buf.ctypes.data, buf.strides[0], kind, w, h, q.ctypes.data, inv, out.ctypes.data, out.strides[0])
        assert rc == 0 and np.all(out[:, 3 * w:] == 777.0)
        assert R.same_bits(out[:, :3 * w].reshape(h, w, 3), want)
    if "zero-column" in case["id"] and w > 2:
        assert not want[:, 2].any() and want[:, 0].any()


def test_rectify_refusals_need_no_context():
    from vision import _vp
    L = _vp.lib()
    w, h, ow, oh = 8, 6, 5, 4
    src = [np.zeros((h, w * 3 + 4), np.uint8) for _ in range(2)]
    xy = [np.zeros((oh, ow, 2), np.int16) for _ in range(2)]
    fr = [np.zeros((oh, ow), np.uint16) for _ in range(2)]
    grey = [np.zeros((oh, ow + 2), np.uint8) for _ in range(2)]
    col = [np.zeros((oh, ow * 3 + 2), np.uint8) for _ in range(2)]

    def call(fn, ctx, **o):
        a = dict(left=_p(src[0]), ls=w * 3 + 4, right=_p(src[1]), rs=w * 3 + 4, w=w, h=h, cn=3, xl=_p(xy[0]), fl=_p(fr[0]), xr=_p(xy[1]), fr=_p(fr[1]), ow=ow, oh=oh,
                 gl=_p(grey[0]), gls=ow + 2, gr=_p(grey[1]), grs=ow + 2, cl=_p(col[0]), cls=ow * 3 + 2, cr=_p(col[1]), crs=ow * 3 + 2)
        a.update(o)
        return fn(*ctx, *a.values())
    for fn, ctx in ((L.vp_rectify_pair_host, ()), (L.vp_rectify_pair_dev, (None,))):
        if not ctx:
            assert call(fn, ctx) == 0 and call(fn, ctx, cl=None, cr=None) == 0
        bad = [dict(w=4097), dict(h=4097), dict(ow=4097), dict(oh=4097), dict(w=0), dict(oh=0), dict(cn=0), dict(cn=2), dict(cn=5),
               dict(left=None), dict(right=None), dict(xl=None), dict(fl=None), dict(xr=None), dict(fr=None), dict(gl=None), dict(gr=None),
               dict(ls=w * 3 - 1), dict(rs=w * 3 - 1), dict(gls=ow - 1), dict(grs=ow - 1), dict(cls=ow * 3 - 1), dict(crs=ow * 3 - 1),
               dict(gl=_p(src[0])), dict(gr=_p(src[1]) + 5), dict(cl=_p(xy[0])), dict(cr=_p(fr[1])), dict(gl=_p(xy[1]) + 3),        # a result on an input
               dict(gr=_p(grey[0]) + 2), dict(cl=_p(grey[0])), dict(cr=_p(col[0]) + 7), dict(cr=_p(grey[1]))]                     # a result on a result
        for o in bad:
            assert call(fn, ctx, **o) == INVALID, (fn.__name__, o)
        assert b"rectify" in L.vp_last_error(None)
    u8 = lambda **o: L.vp_rectify_pair_u8(None, *{**dict(left=_p(src[0]), right=_p(src[1]), w=w, h=h, cn=3, xl=_p(xy[0]), fl=_p(fr[0]), xr=_p(xy[1]), fr=_p(fr[1]), ow=ow, oh=oh,
                                                        gl=_p(grey[0]), gr=_p(grey[1]), cl=None, cr=None), **o}.values())
    for o in (dict(w=4097), dict(cn=2), dict(left=None), dict(xr=None), dict(gr=None), dict(gl=_p(src[0])), dict(gr=_p(grey[0])), dict(w=-1), dict(ow=-1)):
        assert u8(**o) == INVALID, o
    assert u8() == INVALID, "a call that passes every check still needs a context"


def test_reproject_refusals_need_no_context():
    from vision import _vp
    L = _vp.lib()
    w, h = 5, 4
    d16, f32, out = np.zeros((h, w + 1), np.int16), np.zeros((h, w + 1), np.float32), np.zeros((h, 3 * w + 1), np.float32)
    q = np.ascontiguousarray(RC.Q_RIG)

    def call(fn, ctx, **o):
        a = dict(disp=_p(d16), ds=2 * (w + 1), kind=0, w=w, h=h, q=_p(q), inv=-16, out=_p(out), os=4 * (3 * w + 1))
        a.update(o)
        return fn(*ctx, *a.values())
    qnan, qbig = q.copy(), q.copy()
    qnan[1, 2], qbig[3, 3] = np.nan, 1e101
    for fn, ctx in ((L.vp_reproject_to_3d_host, ()), (L.vp_reproject_to_3d_dev, (None,))):
        if not ctx:
            assert call(fn, ctx) == 0 and call(fn, ctx, inv=INT_MIN) == 0 and call(fn, ctx, disp=_p(f32), ds=4 * (w + 1), kind=1, inv=INT_MIN) == 0
        bad = [dict(disp=None), dict(out=None), dict(q=None), dict(kind=2), dict(kind=-1), dict(w=0), dict(h=0), dict(w=4097), dict(h=4097),
               dict(ds=2 * w - 2), dict(ds=2 * w + 1), dict(os=12 * w - 4), dict(os=12 * w + 2), dict(disp=_p(d16) + 1), dict(out=_p(out) + 2),
               dict(q=_p(qnan)), dict(q=_p(qbig)), dict(inv=32768), dict(inv=-32769), dict(disp=_p(f32), ds=4 * (w + 1), kind=1, inv=-16),
               dict(disp=_p(f32), ds=4 * (w + 1) - 2, kind=1, inv=INT_MIN), dict(disp=_p(out), ds=4 * (3 * w + 1), kind=1, inv=INT_MIN), dict(out=_p(d16) + 4, os=12 * w)]
        for o in bad:
            assert call(fn, ctx, **o) == INVALID, (fn.__name__, o)
        assert b"reproject" in L.vp_last_error(None)
    assert L.vp_reproject_to_3d_i16(None, _p(d16), 0, h, _p(q), -16, _p(out)) == INVALID
    assert L.vp_reproject_to_3d_i16(None, _p(d16), w, h, _p(qnan), -16, _p(out)) == INVALID
    assert L.vp_reproject_to_3d_f32(None, None, w, h, _p(q), _p(out)) == INVALID
    assert L.vp_reproject_to_3d_i16(None, _p(d16), w, h, _p(q), -16, _p(out)) == INVALID, "a call that passes every check still needs a context"


def test_python_layer_refuses_before_a_device_is_needed():
    from vision.utils import stereo
    d = np.zeros((4, 5), np.int16)
    with pytest.raises(TypeError):
        stereo.reproject_to_3d(np.zeros((4, 5), np.uint8), RC.Q_RIG)
    with pytest.raises(TypeError):
        stereo.reproject_to_3d(np.zeros((4, 5, 1), np.int16), RC.Q_RIG)
    for q in (np.eye(3), np.full((4, 4), np.nan), RC.Q_RIG * 1e101):
        with pytest.raises(ValueError):
            stereo.reproject_to_3d(d, q)
    with pytest.raises(ValueError):
        stereo.reproject_to_3d(d, RC.Q_RIG, invalid=40000)
    with pytest.raises(ValueError):
        stereo.reproject_to_3d(d.astype(np.float32), RC.Q_RIG, invalid=-16)
    with pytest.raises(TypeError):
        stereo.rectify_pair(np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4, 3), np.uint8), "no table", None)


def test_facade_names_and_argument_order():
    from vision import cv2_facade as f
    from vision.utils.helpers import error
    assert f.CALIB_ZERO_DISPARITY == 1024
    assert list(inspect.signature(f.stereoRectify).parameters) == ["cameraMatrix1", "distCoeffs1", "cameraMatrix2", "distCoeffs2", "imageSize", "R", "T", "R1", "R2",
                                                                   "P1", "P2", "Q", "flags", "alpha", "newImageSize"]
    assert list(inspect.signature(f.reprojectImageTo3D).parameters) == ["disparity", "Q", "_3dImage", "handleMissingValues", "ddepth"]
    assert not hasattr(f, "StereoSGBM_create") and not hasattr(f, "stereoCalibrate")
    d = np.zeros((4, 5), np.float32)
    with pytest.raises(error):
        f.reprojectImageTo3D(d, RC.Q_RIG, handleMissingValues=True)
    with pytest.raises(error):
        f.reprojectImageTo3D(d, RC.Q_RIG, ddepth=f.CV_64F)
    with pytest.raises(error):
        f.reprojectImageTo3D(d, np.eye(3))
    K = np.array([[500.0, 0, 300], [0, 500, 200], [0, 0, 1]])
    out = f.stereoRectify(K, None, K, None, (640, 480), np.eye(3), [-0.1, 0, 0])
    assert len(out) == 7 and out[0].shape == (3, 3) and out[2].shape == (3, 4) and out[4].shape == (4, 4) and len(out[5]) == 4 and len(out[6]) == 4
    with pytest.raises(error):
        f.stereoRectify(K, None, K, None, (640, 480), np.eye(3), [0, 0, 0])
    with pytest.raises(error):
        f.stereoRectify(K, None, K, None, (640, 480), np.eye(3), [-0.1, 0, 0], flags=1)
