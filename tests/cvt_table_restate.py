"""Restatement of the 8-bit colour conversions added beside the first eight codes, in vectorised numpy and independent of
libvp: int64 for the fixed-point paths, np.float32 operation by operation for HLS -> BGR.  descale(x, n) = (x + (1 << (n - 1))) >> n
with numpy's arithmetic shift; results are saturated to 0..255.

The constants are written from memory of OpenCV 4.x (color_yuv.simd.hpp RGB2YCrCb_i / YCrCb2RGB_i, color_lab.cpp RGB2XYZ_i /
XYZ2RGB_i, color_hsv.simd.hpp HLS2RGB_f behind HLS2RGB_b): parity with cv2 is unpinned until tests/test_live_cv2_cvt_table.py runs
somewhere with OpenCV.  This module is what the GPU kernels are compared against.

Every function takes and returns uint8 arrays of shape (..., channels) ((...) for gray)."""
import numpy as np

Y_COEF = (1868, 9617, 4899)                      # blue, green, red, Q14 (the BGR2GRAY coefficients)
YCRCB_FWD = (11682, 9241)                        # (red difference, blue difference) coefficients, Q14
YUV_FWD = (14369, 8061)
YCRCB_INV = (22987, -11698, -5636, 29049)        # r from Cr, g from Cr, g from Cb, b from Cb, Q14
YUV_INV = (18678, -9519, -6472, 33292)           # the same with V for Cr and U for Cb
XYZ_FWD = ((1689, 1465, 739), (871, 2929, 296), (79, 488, 3892))               # rows X, Y, Z applied to (R, G, B), Q12
XYZ_INV = ((13273, -6296, -2042), (-3970, 7684, 170), (228, -836, 4331))       # rows R, G, B applied to (X, Y, Z), Q12


def descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _sat(x):
    return np.clip(x, 0, 255).astype(np.uint8)


def _i64(img):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.shape[-1] == 3
    return img[..., 0].astype(np.int64), img[..., 1].astype(np.int64), img[..., 2].astype(np.int64)


def _ycc_forward(bgr, coef):
    b, g, r = _i64(bgr)
    y = descale(Y_COEF[0] * b + Y_COEF[1] * g + Y_COEF[2] * r, 14)
    cr = descale((r - y) * coef[0] + (128 << 14), 14)
    cb = descale((b - y) * coef[1] + (128 << 14), 14)
    return y, cr, cb


def _ycc_inverse(y, cr, cb, c):
    cr = cr - 128
    cb = cb - 128
    b = y + descale(cb * c[3], 14)
    g = y + descale(cb * c[2] + cr * c[1], 14)
    r = y + descale(cr * c[0], 14)
    return _sat(np.stack([b, g, r], -1))


def bgr2ycrcb(bgr):
    """The existing VP_BGR2YCRCB, restated here for the round trip: Y, Cr, Cb."""
    y, cr, cb = _ycc_forward(bgr, YCRCB_FWD)
    return _sat(np.stack([y, cr, cb], -1))


def bgr2yuv(bgr):
    y, v, u = _ycc_forward(bgr, YUV_FWD)
    return _sat(np.stack([y, u, v], -1))


def ycrcb2bgr(img):
    y, cr, cb = _i64(img)
    return _ycc_inverse(y, cr, cb, YCRCB_INV)


def yuv2bgr(img):
    y, u, v = _i64(img)
    return _ycc_inverse(y, v, u, YUV_INV)


def bgr2xyz(bgr):
    b, g, r = _i64(bgr)
    return _sat(np.stack([descale(m[0] * r + m[1] * g + m[2] * b, 12) for m in XYZ_FWD], -1))


def xyz2bgr(img):
    x, y, z = _i64(img)
    r, g, b = (descale(m[0] * x + m[1] * y + m[2] * z, 12) for m in XYZ_INV)
    return _sat(np.stack([b, g, r], -1))


def hls2bgr(img):
    """HLS2RGB_b over HLS2RGB_f, hue range 180.  Hues from 180 up (not produced by BGR2HLS) wrap by one subtraction of 6 sectors."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.shape[-1] == 3
    f = np.float32
    one, two, six = f(1), f(2), f(6)
    inv255 = one / f(255)
    h = img[..., 0].astype(f) * (six / f(180))
    l = img[..., 1].astype(f) * inv255
    s = img[..., 2].astype(f) * inv255
    p2 = np.where(l <= f(0.5), l * (one + s), (l + s) - l * s).astype(f)
    p1 = (two * l - p2).astype(f)
    h = np.where(h >= six, h - six, h).astype(f)
    fl = np.floor(h)
    sector = fl.astype(np.int64)
    h = (h - fl).astype(f)
    d = (p2 - p1).astype(f)
    t2 = (p1 + d * (one - h)).astype(f)
    t3 = (p1 + d * h).astype(f)
    tab = np.stack([p2, p1, t2, t3], 0)
    sector_data = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])      # (b, g, r) per sector
    out = np.empty(img.shape, np.uint8)
    grey = img[..., 2] == 0
    for c in range(3):
        v = np.take_along_axis(tab, sector_data[sector, c][None], 0)[0]
        v = np.where(grey, l, v).astype(f)
        out[..., c] = np.clip(np.rint(v * f(255)), 0, 255).astype(np.uint8)      # saturate_cast<uchar>: round half to even
    return out


def bgr2gray(bgr):
    b, g, r = _i64(bgr)
    return descale(Y_COEF[0] * b + Y_COEF[1] * g + Y_COEF[2] * r, 14).astype(np.uint8)


# ---- RGB order, alpha, reorders ------------------------------------------------------------------------------------------------------
def swap_rb(img):
    img = np.asarray(img)
    out = img.copy()
    out[..., 0], out[..., 2] = img[..., 2], img[..., 0]
    return out


def rgb_source(fn):
    """the RGB twin of a conversion from BGR"""
    return lambda img: fn(swap_rb(img))


def rgb_result(fn):
    """the RGB twin of a conversion to BGR"""
    return lambda img: swap_rb(fn(img))


def _with_alpha(bgr):
    return np.concatenate([bgr, np.full(bgr.shape[:-1] + (1,), 255, np.uint8)], -1)


NEW_ARITHMETIC = {"BGR2YUV": bgr2yuv, "YUV2BGR": yuv2bgr, "YCRCB2BGR": ycrcb2bgr, "BGR2XYZ": bgr2xyz, "XYZ2BGR": xyz2bgr, "HLS2BGR": hls2bgr}
# every new code whose arithmetic is stated in this file, by its libvp name (vision/_vp.py); the RGB twins of the first eight codes
# (RGB2GRAY apart) are the oracle's function for the BGR code under rgb_source / rgb_result: EXISTING_TWINS
CODES = dict(NEW_ARITHMETIC)
CODES.update({
    "BGR2RGB": swap_rb,
    "RGB2YUV": rgb_source(bgr2yuv), "YUV2RGB": rgb_result(yuv2bgr), "RGB2YCRCB": rgb_source(bgr2ycrcb), "YCRCB2RGB": rgb_result(ycrcb2bgr),
    "RGB2XYZ": rgb_source(bgr2xyz), "XYZ2RGB": rgb_result(xyz2bgr), "HLS2RGB": rgb_result(hls2bgr), "RGB2GRAY": rgb_source(bgr2gray),
    "BGRA2BGR": lambda a: np.ascontiguousarray(a[..., :3]),
    "RGBA2BGR": lambda a: np.ascontiguousarray(a[..., 2::-1]),
    "BGR2BGRA": _with_alpha,
    "BGR2RGBA": lambda a: _with_alpha(swap_rb(a)),
    "BGRA2RGBA": swap_rb,
    "GRAY2BGRA": lambda g: _with_alpha(np.stack([g, g, g], -1)),
    "BGRA2GRAY": lambda a: bgr2gray(a[..., :3]),
    "RGBA2GRAY": lambda a: bgr2gray(a[..., 2::-1]),
})
# libvp name -> (name of the oracle / restatement function of the BGR code, which side is RGB)
EXISTING_TWINS = {"RGB2HSV": ("bgr2hsv", "source"), "HSV2RGB": ("hsv2bgr", "result"), "RGB2HLS": ("bgr2hls", "source"),
                  "RGB2LAB": ("bgr2lab", "source"), "LAB2RGB": ("lab2bgr", "result")}
SOURCE_CHANNELS = {"GRAY2BGRA": 1, "BGRA2BGR": 4, "RGBA2BGR": 4, "BGRA2RGBA": 4, "BGRA2GRAY": 4, "RGBA2GRAY": 4}      # 3 otherwise


def all_colours():
    """(4096, 4096, 3): every 8-bit triple once."""
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
