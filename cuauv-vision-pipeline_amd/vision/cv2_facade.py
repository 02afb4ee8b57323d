"""A narrow `cv2` look-alike for module files that call OpenCV directly (modules/bins.py:13-75 and the colour /
morphology lines of modules/preprocessor.py:52-129), so they run where no OpenCV exists.

`install()` registers this module as `cv2` ONLY when a real cv2 cannot be imported — a real OpenCV is never shadowed.
Image arithmetic (cvtColor, inRange, erode/dilate/morphologyEx, findContours, connectedComponentsWithStats) goes to
libvp (HIP); small polygon maths (moments, contourArea, arcLength, minAreaRect, boxPoints, approxPolyDP) is host numpy, as it is
CPU code in OpenCV too.  The element-wise operators (bitwise_*, add / subtract / absdiff, LUT, split / merge / extractChannel,
countNonZero) are host numpy for numpy images and libvp kernels as soon as one image operand is a DeviceMat.  Anything else
raises AttributeError like a missing cv2 symbol would.

An image operator's launch lives in the mirror (vision.utils.transform / color), never here: a name of this module is cv2's argument
order, cv2's own rejections, `_into(dst, ...)` and `_gather`, which turns what the mirror refuses into `error`."""
import math
import sys

import numpy as np

from vision import _vp
from vision.utils import color as _color
from vision.utils import draw as _draw
from vision.utils import feature as _feature
from vision.utils import transform as _transform
from vision.utils.helpers import as_cv2_error as _gather, error, image_source as _image_source, packed_source as _device_source  # noqa: F401

COLOR_BGR2LAB, COLOR_BGR2HSV, COLOR_BGR2GRAY, COLOR_GRAY2BGR, COLOR_HSV2BGR = 44, 40, 6, 8, 54     # cv2's own enum values
COLOR_BGR2YCrCb, COLOR_BGR2YCR_CB, COLOR_BGR2HLS = 36, 36, 52
COLOR_LAB2BGR = COLOR_Lab2BGR = 56
COLOR_BGR2BGRA, COLOR_BGRA2BGR, COLOR_RGBA2RGB, COLOR_BGR2RGBA, COLOR_RGBA2BGR, COLOR_BGRA2RGB = 0, 1, 1, 2, 3, 3
COLOR_BGR2RGB, COLOR_RGB2BGR, COLOR_BGRA2RGBA, COLOR_RGBA2BGRA = 4, 4, 5, 5
COLOR_RGB2GRAY, COLOR_GRAY2BGRA, COLOR_BGRA2GRAY, COLOR_RGBA2GRAY = 7, 9, 10, 11
COLOR_BGR2XYZ, COLOR_RGB2XYZ, COLOR_XYZ2BGR, COLOR_XYZ2RGB = 32, 33, 34, 35
COLOR_RGB2YCrCb, COLOR_RGB2YCR_CB, COLOR_YCrCb2BGR, COLOR_YCR_CB2BGR, COLOR_YCrCb2RGB, COLOR_YCR_CB2RGB = 37, 37, 38, 38, 39, 39
COLOR_RGB2HSV, COLOR_RGB2Lab, COLOR_RGB2LAB, COLOR_RGB2HLS, COLOR_HSV2RGB = 41, 45, 45, 53, 55
COLOR_Lab2RGB, COLOR_LAB2RGB, COLOR_HLS2BGR, COLOR_HLS2RGB = 57, 57, 60, 61
COLOR_BGR2YUV, COLOR_RGB2YUV, COLOR_YUV2BGR, COLOR_YUV2RGB = 82, 83, 84, 85
COLOR_BGR2Luv, COLOR_BGR2LUV = 50, 50     # named by modules/preprocessor.py:76; see DESIGN.md section 7 for what the stand-in does with it
MORPH_RECT, MORPH_CROSS, MORPH_ELLIPSE = 0, 1, 2
MORPH_ERODE, MORPH_DILATE, MORPH_OPEN, MORPH_CLOSE, MORPH_GRADIENT = 0, 1, 2, 3, 4
RETR_EXTERNAL, RETR_LIST, RETR_CCOMP, RETR_TREE = 0, 1, 2, 3
CHAIN_APPROX_NONE, CHAIN_APPROX_SIMPLE = 1, 2
CC_STAT_LEFT, CC_STAT_TOP, CC_STAT_WIDTH, CC_STAT_HEIGHT, CC_STAT_AREA = 0, 1, 2, 3, 4
CV_8U = 0
ADAPTIVE_THRESH_MEAN_C, ADAPTIVE_THRESH_GAUSSIAN_C = 0, 1
THRESH_BINARY, THRESH_BINARY_INV, THRESH_TRUNC, THRESH_TOZERO, THRESH_TOZERO_INV = 0, 1, 2, 3, 4
THRESH_MASK, THRESH_OTSU, THRESH_TRIANGLE = 7, 8, 16
CV_32S = 4
CV_16S, CV_32F, CV_64F = 3, 5, 6
FILTER_SCHARR = -1
CV_PI = math.pi
HOUGH_GRADIENT, HOUGH_GRADIENT_ALT = 3, 4


class UMat:   # only so that `from cv2 import UMat` and isinstance checks work
    def __init__(self, arr):
        self._arr = np.asarray(arr)

    def get(self):
        return self._arr


_CVT = {COLOR_BGR2LAB: _color.bgr_to_lab, COLOR_BGR2HSV: _color.bgr_to_hsv, COLOR_BGR2GRAY: _color.bgr_to_gray,
        COLOR_GRAY2BGR: _color.gray_to_bgr, COLOR_HSV2BGR: _color.hsv_to_bgr, COLOR_BGR2YCrCb: _color.bgr_to_ycrcb,
        COLOR_BGR2HLS: _color.bgr_to_hls, COLOR_LAB2BGR: _color.lab_to_bgr,
        COLOR_BGR2YUV: _color.bgr_to_yuv, COLOR_YUV2BGR: _color.yuv_to_bgr, COLOR_BGR2XYZ: _color.bgr_to_xyz, COLOR_XYZ2BGR: _color.xyz_to_bgr,
        COLOR_YCrCb2BGR: _color.ycrcb_to_bgr, COLOR_HLS2BGR: _color.hls_to_bgr}
# the RGB-order, alpha and reorder codes have no name in utils/color.py: straight to their libvp codes
_CVT.update({cv: _color._convert_colorspace(vp) for cv, vp in (
    (COLOR_BGR2BGRA, _vp.BGR2BGRA), (COLOR_BGRA2BGR, _vp.BGRA2BGR), (COLOR_BGR2RGBA, _vp.BGR2RGBA), (COLOR_RGBA2BGR, _vp.RGBA2BGR),
    (COLOR_BGR2RGB, _vp.BGR2RGB), (COLOR_BGRA2RGBA, _vp.BGRA2RGBA), (COLOR_RGB2GRAY, _vp.RGB2GRAY), (COLOR_GRAY2BGRA, _vp.GRAY2BGRA),
    (COLOR_BGRA2GRAY, _vp.BGRA2GRAY), (COLOR_RGBA2GRAY, _vp.RGBA2GRAY), (COLOR_RGB2XYZ, _vp.RGB2XYZ), (COLOR_XYZ2RGB, _vp.XYZ2RGB),
    (COLOR_RGB2YCrCb, _vp.RGB2YCRCB), (COLOR_YCrCb2RGB, _vp.YCRCB2RGB), (COLOR_RGB2HSV, _vp.RGB2HSV), (COLOR_HSV2RGB, _vp.HSV2RGB),
    (COLOR_RGB2Lab, _vp.RGB2LAB), (COLOR_Lab2RGB, _vp.LAB2RGB), (COLOR_RGB2HLS, _vp.RGB2HLS), (COLOR_HLS2RGB, _vp.HLS2RGB),
    (COLOR_RGB2YUV, _vp.RGB2YUV), (COLOR_YUV2RGB, _vp.YUV2RGB))})


def cvtColor(src, code):
    if code not in _CVT:
        raise error(f"cvtColor code {code} is outside the accelerated path")
    return _CVT[code](src)[0]


def split(m):
    """cv2.split.  A uint8 DeviceMat of 2..4 channels gives DeviceMat planes (libvp vp_split_u8_dev) that share one allocation, each
    starting at a multiple of 256 bytes; a single-channel one gives a one-element tuple with a device copy."""
    from vision.devmat import DeviceMat, _DevBuf
    from vision.utils.helpers import as_mat
    m = as_mat(m)
    if isinstance(m, DeviceMat) and m.dtype == np.uint8 and m.size and (m.ndim == 2 or (m.ndim == 3 and 1 <= m.shape[2] <= 4)):
        ctx = _vp.default_context()
        m.refresh_device(ctx)
        h, w = m.shape[:2]
        cn = 1 if m.ndim == 2 else m.shape[2]
        if cn == 1:
            out = DeviceMat(ctx, (h, w))
            _vp.check(_vp.lib().vp_memcpy_d2d_async(ctx.handle, out.dev_ptr, m.dev_ptr, h * w), ctx.handle)
            return (out,)
        pitch = (h * w + 255) & ~255
        buf = _DevBuf(ctx, pitch * cn)
        planes = tuple(DeviceMat.over_buffer(ctx, buf, c * pitch, (h, w), np.uint8) for c in range(cn))
        ptrs = [p.dev_ptr for p in planes] + [None] * (4 - cn)
        _vp.check(_vp.lib().vp_split_u8_dev(ctx.handle, m.dev_ptr, h * w, cn, *ptrs), ctx.handle)
        return planes
    m = np.asarray(m)
    return tuple(np.ascontiguousarray(m[:, :, c]) for c in range(m.shape[2])) if m.ndim == 3 else (m.copy(),)


def merge(mv):
    """cv2.merge.  2..4 uint8 planes of one 2-D shape of which at least one is a DeviceMat give a DeviceMat (libvp vp_merge_u8_dev;
    numpy planes are uploaded)."""
    from vision.devmat import DeviceMat, finish_uploads
    from vision.utils.helpers import as_mat
    mv = [as_mat(p) for p in mv]
    if any(isinstance(p, DeviceMat) for p in mv) and 2 <= len(mv) <= 4 and \
            all(isinstance(p, (np.ndarray, DeviceMat)) and p.dtype == np.uint8 and p.ndim == 2 and p.size and tuple(p.shape) == tuple(mv[0].shape) for p in mv):
        ctx = _vp.default_context()
        up = []
        try:
            planes = [_on_device(ctx, p, up) for p in mv]
            h, w = planes[0].shape
            out = DeviceMat(ctx, (h, w, len(planes)))
            ptrs = [p.dev_ptr for p in planes] + [None] * (4 - len(planes))
            _vp.check(_vp.lib().vp_merge_u8_dev(ctx.handle, *ptrs, h * w, len(planes), out.dev_ptr), ctx.handle)
        finally:
            finish_uploads(ctx, up)
        return out
    return np.ascontiguousarray(np.dstack([np.asarray(p) for p in mv]))


def extractChannel(src, coi):
    """cv2.extractChannel: plane `coi` of an image; of a uint8 DeviceMat on the device (vp_split_u8_dev with one destination)."""
    from vision.devmat import DeviceMat
    from vision.utils.helpers import as_mat
    src = as_mat(src)
    if not isinstance(src, (np.ndarray, DeviceMat)) or src.ndim not in (2, 3) or src.size == 0:
        raise error("extractChannel: expected a non-empty image")
    cn = 1 if src.ndim == 2 else src.shape[2]
    coi = int(coi)
    if not 0 <= coi < cn:
        raise error("extractChannel: the channel index is out of range")
    if isinstance(src, DeviceMat) and src.dtype == np.uint8 and cn <= 4:
        ctx = _vp.default_context()
        src.refresh_device(ctx)
        h, w = src.shape[:2]
        out = DeviceMat(ctx, (h, w))
        if cn == 1:
            _vp.check(_vp.lib().vp_memcpy_d2d_async(ctx.handle, out.dev_ptr, src.dev_ptr, h * w), ctx.handle)
        else:
            ptrs = [out.dev_ptr if c == coi else None for c in range(4)]
            _vp.check(_vp.lib().vp_split_u8_dev(ctx.handle, src.dev_ptr, h * w, cn, *ptrs), ctx.handle)
        return out
    src = np.asarray(src)
    return src.copy() if src.ndim == 2 else np.ascontiguousarray(src[:, :, coi])


def countNonZero(src):
    """cv2.countNonZero (single channel only): of a uint8 DeviceMat on the device (vp_count_nonzero_u8_dev), numpy input by numpy."""
    from vision.devmat import DeviceMat
    from vision.utils.helpers import as_mat
    src = as_mat(src)
    if not isinstance(src, (np.ndarray, DeviceMat)) or src.ndim not in (1, 2, 3) or (src.ndim == 3 and src.shape[2] != 1):
        raise error("countNonZero: expected a single-channel image")
    if isinstance(src, DeviceMat) and src.dtype == np.uint8 and src.size:
        ctx = _vp.default_context()
        src.refresh_device(ctx)
        n = _vp.C.c_uint64(0)
        _vp.check(_vp.lib().vp_count_nonzero_u8_dev(ctx.handle, src.dev_ptr, src.size, _vp.C.byref(n)), ctx.handle)
        return int(n.value)
    return int(np.count_nonzero(np.asarray(src)))


def inRange(src, lowerb, upperb):
    return _color.range_threshold(src, lowerb, upperb)


def getStructuringElement(shape, ksize):
    return _transform._structuring_element(int(shape), int(ksize[0]), int(ksize[1]))


BORDER_CONSTANT = 0
BORDER_REPLICATE = 1
BORDER_REFLECT = 2
BORDER_WRAP = 3
BORDER_REFLECT_101 = BORDER_REFLECT101 = 4
BORDER_DEFAULT = 4
BORDER_ISOLATED = 16


def _into(dst, result):
    """cv2's optional `dst` argument: the result is also written into it when it has the right shape and type (cv2 reallocates
    otherwise, which a caller-owned numpy array cannot do: the returned array is the result either way)."""
    if dst is not None:
        from vision.devmat import to_host
        d = to_host(dst)
        r = np.asarray(result)
        if isinstance(d, np.ndarray) and d.shape == r.shape and d.dtype == r.dtype and d.flags.writeable:
            np.copyto(d, r)
            return dst
    return result


def _default_border_only(name, borderType, borderValue):
    # cv2's default for morphology: BORDER_CONSTANT with morphologyDefaultBorderValue() = "outside never wins"
    if borderType not in (None, BORDER_CONSTANT) or borderValue is not None:
        raise error(f"{name}: only the default border (constant, morphologyDefaultBorderValue) is on the accelerated path")


# positional order as in cv2: (src, kernel, dst, anchor, iterations, borderType, borderValue)
def erode(src, kernel, dst=None, anchor=None, iterations=1, borderType=None, borderValue=None):
    _default_border_only("erode", borderType, borderValue)
    return _into(dst, _transform._morph(_vp.MORPH_ERODE, src, kernel, iterations, anchor if anchor is not None else (-1, -1)))


def dilate(src, kernel, dst=None, anchor=None, iterations=1, borderType=None, borderValue=None):
    _default_border_only("dilate", borderType, borderValue)
    return _into(dst, _transform._morph(_vp.MORPH_DILATE, src, kernel, iterations, anchor if anchor is not None else (-1, -1)))


# (src, op, kernel, dst, anchor, iterations, borderType, borderValue)
def morphologyEx(src, op, kernel, dst=None, anchor=None, iterations=1, borderType=None, borderValue=None):
    _default_border_only("morphologyEx", borderType, borderValue)
    return _into(dst, _transform._morph(int(op), src, kernel, iterations, anchor if anchor is not None else (-1, -1)))


def findContours(image, mode, method):
    """-> (contours, hierarchy).  RETR_CCOMP / RETR_TREE: cv2's hierarchy, int32 (1, N, 4) [next, prev, first_child, parent], and
    ((), None) without contours; RETR_EXTERNAL / RETR_LIST: the hierarchy is None (they are flat)."""
    mode, method = int(mode), int(method)
    if mode not in (RETR_EXTERNAL, RETR_LIST, RETR_CCOMP, RETR_TREE):
        raise error(f"findContours: retrieval mode {mode} is not implemented (RETR_FLOODFILL is out of scope)")
    if mode in (RETR_CCOMP, RETR_TREE):
        contours, hierarchy = _feature.find_contours(image, mode, method, with_hierarchy=True)
        return (contours if len(contours) else ()), hierarchy
    return _feature.find_contours(image, mode, method), None


def connectedComponentsWithStats(image, connectivity=8, ltype=CV_32S):
    if connectivity != 8:
        raise error("only 8-connectivity is implemented")
    if ltype != CV_32S:
        raise error("only CV_32S labels are implemented")
    cap = 4096
    while True:                                    # stats and centroids always have one row per label, as in cv2
        n, labels, stats, cent = _feature.connected_components(image, max_labels=cap)
        if n <= cap:
            return n, labels, stats, cent
        cap = n


def moments(array, binaryImage=False):
    """cv2.moments, cv2's 24-key dictionary.  An (N, 2) or (N, 1, 2) int32 or float32 array is a contour (contourMoments' float64 loop,
    host code; binaryImage is ignored, as in cv2); a 2-D uint8 array or DeviceMat is an image, summed on the GPU in exact integers."""
    from vision.devmat import DeviceMat
    from vision.utils.helpers import as_mat
    a = as_mat(array)
    if isinstance(a, DeviceMat):
        if a.dtype == np.uint8 and (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 1)) and a.size:
            return _feature.moments_dict(_gather("moments", _feature.image_moments, a, bool(binaryImage)))
    elif isinstance(a, np.ndarray):
        if a.dtype in (np.int32, np.float32) and ((a.ndim == 2 and a.shape[1] == 2) or (a.ndim == 3 and a.shape[1:] == (1, 2))):
            return _feature.moments_dict(_feature.contour_moments(a))
        if a.dtype == np.uint8 and a.ndim == 2 and a.size:
            return _feature.moments_dict(_gather("moments", _feature.image_moments, a, bool(binaryImage)))
    raise error("moments: only int32 / float32 contours and single-channel uint8 images are on the accelerated path")


def HuMoments(m, hu=None):
    """cv2.HuMoments of a moments dictionary: float64 (7, 1)."""
    if not isinstance(m, dict) or any(k not in m for k in _feature.MOMENT_FIELDS[17:]):
        raise error("HuMoments: expected the dictionary cv2.moments returns")
    return _into(hu, _feature.hu_moments(m).reshape(7, 1))


def contourArea(contour, oriented=False):
    pts = np.asarray(contour).reshape(-1, 2).astype(np.float64)
    if len(pts) == 0:
        return 0.0
    x, y = pts[:, 0], pts[:, 1]
    a = 0.5 * float(np.sum(np.roll(x, 1) * y - np.roll(y, 1) * x))
    return a if oriented else abs(a)


def arcLength(curve, closed):
    """imgproc/src/shapedescr.cpp arcLength: segment lengths in float32, summed in float64."""
    pts = np.asarray(curve).reshape(-1, 2).astype(np.float32)
    if len(pts) <= 1:
        return 0.0
    prev = pts[-1] if closed else pts[0]
    total = 0.0
    for i in range(0 if closed else 1, len(pts)):
        d = pts[i] - prev
        total += float(np.sqrt(np.float32(d[0] * d[0] + d[1] * d[1])))
        prev = pts[i]
    return total


def _convex_hull_py(pts):
    pts = sorted(set(map(tuple, pts.tolist())))
    if len(pts) <= 2:
        return np.array(pts, np.float64)

    def cross(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return np.array(lower[:-1] + upper[:-1], np.float64)


def _convex_hull(points):
    """Monotone-chain hull as float64 (k, 2): integer points (contours) through libvp's exact host routine, anything else in Python."""
    p = np.asarray(points).reshape(-1, 2)
    if np.issubdtype(p.dtype, np.integer) and len(p) and np.abs(p).max(initial=0) < 2**31:
        p32 = np.ascontiguousarray(p, np.int32)
        out = np.empty_like(p32)
        n = _vp.C.c_int(0)
        _vp.check(_vp.lib().vp_convex_hull_i32(p32.ctypes.data, len(p32), out.ctypes.data, _vp.C.byref(n)))
        return out[:n.value].astype(np.float64)
    return _convex_hull_py(p.astype(np.float64))


def minAreaRect(points):
    """Minimum-area enclosing rectangle by rotating calipers over the convex hull: ((cx, cy), (w, h), angle in degrees).
    Angle convention of OpenCV >= 4.5.1: in (0, 90], width measured along the edge that defines the angle."""
    p = np.asarray(points).reshape(-1, 2)
    # contours: hull and calipers in libvp's host routine (the doubles of _min_area_rect_loop, statement by statement).  What
    # find_contours returns is int32 already: no range check, no copy (numpy calls on a handful of points cost more than the calipers)
    if len(p) and (p.dtype == np.int32 or (np.issubdtype(p.dtype, np.integer) and np.abs(p).max(initial=0) < 2**31)):
        p32 = p if (p.dtype == np.int32 and p.flags.c_contiguous) else np.ascontiguousarray(p, np.int32)
        out = (_vp.C.c_float * 5)()
        _vp.check(_vp.lib().vp_min_area_rect_i32(p32.ctypes.data, len(p32), out))
        return (out[0], out[1]), (out[2], out[3]), out[4]
    hull = _convex_hull(points)
    if len(hull) == 0:
        return (0.0, 0.0), (0.0, 0.0), 0.0
    if len(hull) == 1:
        return (float(hull[0, 0]), float(hull[0, 1])), (0.0, 0.0), 90.0
    n = len(hull)
    # every edge at once (columns): the same products and sums as edge by edge, the first edge of minimal area wins
    e = (np.roll(hull, -1, axis=0) - hull)[: (n if n > 2 else 1)]
    ln = np.array([math.sqrt(x * x + y * y) for x, y in e.tolist()])
    keep = ln != 0
    if not keep.any():
        return (float(hull[0, 0]), float(hull[0, 1])), (0.0, 0.0), 90.0
    e, ln = e[keep], ln[keep]
    ux, uy = e[:, 0] / ln, e[:, 1] / ln
    hx, hy = hull[:, 0][:, None], hull[:, 1][:, None]
    a = hx * ux + hy * uy
    b = -hx * uy + hy * ux
    amax, amin, bmax, bmin = a.max(0), a.min(0), b.max(0), b.min(0)
    wds, hts = amax - amin, bmax - bmin
    k = int(np.argmin(wds * hts))
    ca, cb = (amax[k] + amin[k]) / 2, (bmax[k] + bmin[k]) / 2
    uxk, uyk = float(ux[k]), float(uy[k])
    cx, cy, wd, ht, ang = ca * uxk - cb * uyk, ca * uyk + cb * uxk, float(wds[k]), float(hts[k]), math.degrees(math.atan2(uyk, uxk))
    while ang <= 0:
        ang += 90
        wd, ht = ht, wd
    while ang > 90:
        ang -= 90
        wd, ht = ht, wd
    return (float(np.float32(cx)), float(np.float32(cy))), (float(np.float32(wd)), float(np.float32(ht))), float(np.float32(ang))


def _min_area_rect_loop(points):
    """The same statements edge by edge (the form the vectorised one is tested against)."""
    pts = np.asarray(points).reshape(-1, 2).astype(np.float64)
    hull = _convex_hull_py(pts)
    if len(hull) == 0:
        return (0.0, 0.0), (0.0, 0.0), 0.0
    if len(hull) == 1:
        return (float(hull[0, 0]), float(hull[0, 1])), (0.0, 0.0), 90.0
    best = None
    n = len(hull)
    for i in range(n if n > 2 else 1):
        e = hull[(i + 1) % n] - hull[i]
        ln = math.sqrt(e[0] * e[0] + e[1] * e[1])     # (exact under the root for integer points)
        if ln == 0:
            continue
        ux, uy = e[0] / ln, e[1] / ln
        a = hull[:, 0] * ux + hull[:, 1] * uy
        b = -hull[:, 0] * uy + hull[:, 1] * ux
        wd, ht = a.max() - a.min(), b.max() - b.min()
        if best is None or wd * ht < best[0]:
            ca, cb = (a.max() + a.min()) / 2, (b.max() + b.min()) / 2
            best = (wd * ht, (ca * ux - cb * uy, ca * uy + cb * ux), wd, ht, math.degrees(math.atan2(uy, ux)))
    _, (cx, cy), wd, ht, ang = best
    while ang <= 0:
        ang += 90
        wd, ht = ht, wd
    while ang > 90:
        ang -= 90
        wd, ht = ht, wd
    return (float(np.float32(cx)), float(np.float32(cy))), (float(np.float32(wd)), float(np.float32(ht))), float(np.float32(ang))


def minEnclosingCircle(points):
    """cv2.minEnclosingCircle for integer points: ((cx, cy), radius) of the smallest enclosing circle (vision.utils.feature.
    min_enclosing_circle: exact support set, no safety margin on the radius)."""
    try:
        return _feature.min_enclosing_circle(points)
    except ValueError as e:
        raise error(str(e))


def boxPoints(box):
    """Corners of a rotated rect, in OpenCV's order (RotatedRect::points): bottom-left, top-left, top-right, bottom-right."""
    (cx, cy), (w, h), ang = box
    a = math.radians(ang)
    b, c = math.cos(a) * 0.5, math.sin(a) * 0.5
    p0 = (cx - c * h - b * w, cy + b * h - c * w)   # a = sin*0.5, b = cos*0.5 in OpenCV's source
    p1 = (cx + c * h - b * w, cy - b * h - c * w)
    p2 = (2 * cx - p0[0], 2 * cy - p0[1])
    p3 = (2 * cx - p1[0], 2 * cy - p1[1])
    return np.array([p0, p1, p2, p3], np.float32)


def approxPolyDP(curve, epsilon, closed):
    """Douglas-Peucker on the point list (closed curves are split at the two mutually farthest points)."""
    pts = np.asarray(curve).reshape(-1, 2).astype(np.float64)
    n = len(pts)
    if n <= 2:
        return np.asarray(curve).reshape(-1, 1, 2).copy()

    def rdp(lo, hi, keep):
        a, b = pts[lo], pts[hi % n]
        idx = [i % n for i in range(lo + 1, hi)]
        if not idx:
            return
        d = b - a
        ln = math.hypot(d[0], d[1])
        seg = pts[idx]
        dist = np.abs(d[0] * (seg[:, 1] - a[1]) - d[1] * (seg[:, 0] - a[0])) / ln if ln > 0 else np.hypot(seg[:, 0] - a[0], seg[:, 1] - a[1])
        k = int(np.argmax(dist))
        if dist[k] > epsilon:
            m = lo + 1 + k
            keep.add(m % n)
            rdp(lo, m, keep)
            rdp(m, hi, keep)
    keep = set()
    if closed:
        d0 = np.hypot(pts[:, 0] - pts[0, 0], pts[:, 1] - pts[0, 1])
        far = int(np.argmax(d0))
        d1 = np.hypot(pts[:, 0] - pts[far, 0], pts[:, 1] - pts[far, 1])
        start = int(np.argmax(d1))
        keep.update((start, far))
        a, b = sorted((start, far))
        rdp(a, b, keep)
        rdp(b, a + n, keep)
    else:
        keep.update((0, n - 1))
        rdp(0, n - 1, keep)
    out = np.asarray(curve).reshape(-1, 2)[sorted(keep)]
    return out.reshape(-1, 1, 2).copy()


def addWeighted(src1, alpha, src2, beta, gamma, dst=None, dtype=-1):
    """saturate_cast<uchar>(src1*alpha + src2*beta + gamma) with round-half-even (modules/bins.py:20), every step a double.  Two uint8
    images of one shape stay on the device (libvp vp_add_weighted_u8_dev: the same doubles) and the result is computed when something
    reads it - bins.py draws into the overlay only when it has found rectangles, and posts it only when posts are on."""
    from vision.devmat import DeviceMat, defer_enabled, finish_uploads, lazy_enabled
    from vision.utils.helpers import as_mat, device_image
    a, b = as_mat(src1), as_mat(src2)
    on_dev = (lazy_enabled() or isinstance(a, DeviceMat) or isinstance(b, DeviceMat)) and dtype in (-1, CV_8U) and \
        all(isinstance(m, (np.ndarray, DeviceMat)) and m.dtype == np.uint8 and m.ndim in (2, 3) and m.size for m in (a, b)) and \
        tuple(a.shape) == tuple(b.shape)
    if not on_dev:
        acc = np.asarray(a, np.float64) * alpha + np.asarray(b, np.float64) * beta + gamma
        return _into(dst, np.clip(np.rint(acc), 0, 255).astype(np.uint8))
    ctx = _vp.default_context()
    up = []
    try:
        da = device_image(ctx, a, 0, pending=up)
        db = device_image(ctx, b, 0, pending=up)
        fa, fb, fg = float(alpha), float(beta), float(gamma)
        n = int(np.prod(da.shape))

        def run(out, da=da, db=db):
            _vp.check(_vp.lib().vp_add_weighted_u8_dev(ctx.handle, da.dev_ptr, fa, db.dev_ptr, fb, fg, n, out.dev_ptr), ctx.handle)
        if defer_enabled() and not (da.host_escaped or db.host_escaped):
            out = DeviceMat.deferred(ctx, da.shape, np.uint8, False, (da, db), run)
        else:
            out = DeviceMat(ctx, da.shape)
            run(out)
    finally:
        finish_uploads(ctx, up)
    return _into(dst, out)


# ---- element-wise operators (libvp vp_elementwise.hip) ------------------------------------------------------------------------------
# numpy in gives numpy out through host numpy; one DeviceMat among the image operands keeps the work and the result on the device.

def _on_device(ctx, m, pending):
    """DeviceMat of a checked uint8 image on ctx (a numpy image is uploaded, shape kept)."""
    from vision.devmat import DeviceMat
    if isinstance(m, DeviceMat):
        m.refresh_device(ctx)
        return m
    return DeviceMat.from_host(ctx, m, pending=pending)


def _is_image(x):
    from vision.devmat import DeviceMat
    return isinstance(x, DeviceMat) or (isinstance(x, np.ndarray) and x.ndim >= 2)


def _check_images(name, *mats):
    """What cv2 rejects of the image operands of an element-wise operator, and what is outside this path."""
    for m in mats:
        if m.ndim not in (2, 3) or m.size == 0:
            raise error(f"{name}: expected non-empty (h, w) or (h, w, c) images")
        if m.dtype != np.uint8:
            raise error(f"{name}: only uint8 images are on the accelerated path")
        if tuple(m.shape) != tuple(mats[0].shape):
            raise error(f"{name}: the images differ in size or in the number of channels")


def _scalar_per_channel(name, s, cn):
    """cv2's scalar operand as cn float64 values: one number (every channel, as `add` always did here) or up to four, one per channel."""
    try:
        v = np.asarray(s, dtype=np.float64).ravel()
    except (TypeError, ValueError):
        raise error(f"{name}: an operand is neither an image nor a scalar") from None
    if np.ndim(s) == 0:
        return np.full(cn, float(v[0]))
    if not cn <= v.size <= 4:
        raise error(f"{name}: the scalar needs one value per channel")
    return v[:cn].copy()


def _arith_statement(op, a, s, image_first):
    """The float64 statement of image-with-scalar arithmetic: the scalar is a double, the result saturate_cast (round half even)."""
    a = a.astype(np.float64)
    if op == _vp.ARITH_ADD:
        acc = a + s
    elif op == _vp.ARITH_SUB:
        acc = a - s if image_first else s - a
    else:
        acc = np.abs(a - s)
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def _launch(ctx, shape, inputs, run, binary=False):
    """The result of an element-wise operator: computed when first needed (DeviceMat.deferred) under the rule addWeighted follows."""
    from vision.devmat import DeviceMat, defer_enabled
    if defer_enabled() and not any(x.host_escaped for x in inputs):
        return DeviceMat.deferred(ctx, shape, np.uint8, binary, inputs, run)
    out = DeviceMat(ctx, shape, binary=binary)
    run(out)
    return out


def _lut_on_device(src, tables):
    """tables: uint8 (cn, 256) for the cn interleaved channels of src, or (1, 256) for every byte."""
    from vision.devmat import finish_uploads
    ctx = _vp.default_context()
    up = []
    try:
        d = _on_device(ctx, src, up)
        tables = np.ascontiguousarray(tables, np.uint8)
        n = int(d.size)

        def run(out, d=d):
            _vp.check(_vp.lib().vp_lut_u8_dev(ctx.handle, d.dev_ptr, n, len(tables), _vp.ptr(tables), out.dev_ptr), ctx.handle)
        return _launch(ctx, d.shape, (d,), run)
    finally:
        finish_uploads(ctx, up)


def _arith(name, op, src1, src2, dst):
    from vision.devmat import DeviceMat, finish_uploads
    from vision.utils.helpers import as_mat
    a, b = as_mat(src1), as_mat(src2)
    ia, ib = _is_image(a), _is_image(b)
    if not (ia or ib):
        raise error(f"{name}: at least one operand must be an image")
    if ia and ib:
        _check_images(name, a, b)
        if not (isinstance(a, DeviceMat) or isinstance(b, DeviceMat)):
            x, y = a.astype(np.int32), b.astype(np.int32)
            r = x + y if op == _vp.ARITH_ADD else x - y if op == _vp.ARITH_SUB else np.abs(x - y)
            return _into(dst, np.clip(r, 0, 255).astype(np.uint8))
        ctx = _vp.default_context()
        up = []
        try:
            da, db = _on_device(ctx, a, up), _on_device(ctx, b, up)
            n = int(da.size)

            def run(out, da=da, db=db):
                _vp.check(_vp.lib().vp_arith_u8_dev(ctx.handle, op, da.dev_ptr, db.dev_ptr, n, out.dev_ptr), ctx.handle)
            return _into(dst, _launch(ctx, da.shape, (da, db), run))
        finally:
            finish_uploads(ctx, up)
    img, s = (a, b) if ia else (b, a)
    _check_images(name, img)
    cn = 1 if img.ndim == 2 else img.shape[2]
    if cn > 4:
        raise error(f"{name}: at most 4 channels with a scalar operand")
    per_channel = np.ndim(s) != 0
    s = _scalar_per_channel(name, s, cn)
    if isinstance(img, np.ndarray):                      # host numpy, as ever: cv2 adds the scalar as a double, then saturate_cast
        return _into(dst, _arith_statement(op, img, (s if img.ndim == 3 else s[0]) if per_channel else float(s[0]), ia))
    # a device image: the same statement on the 256 values a byte can take, per channel, applied as a table (vp_lut_u8_dev)
    tables = np.stack([_arith_statement(op, np.arange(256), float(v), ia) for v in (s if per_channel else s[:1])])
    return _into(dst, _lut_on_device(img, tables))


def add(src1, src2, dst=None):
    """cv2.add with saturation; one operand may be a scalar or a per-channel tuple (modules/preprocessor.py:90-103 adds a bias to a
    channel).  Two images, one of them a DeviceMat: libvp vp_arith_u8_dev; a DeviceMat and a scalar: a table (vp_lut_u8_dev)."""
    return _arith("add", _vp.ARITH_ADD, src1, src2, dst)


def subtract(src1, src2, dst=None):
    """cv2.subtract (src1 - src2, saturated at 0); either operand may be the scalar."""
    return _arith("subtract", _vp.ARITH_SUB, src1, src2, dst)


def absdiff(src1, src2, dst=None):
    """cv2.absdiff."""
    return _arith("absdiff", _vp.ARITH_ABSDIFF, src1, src2, dst)


def _bitwise(name, op, src1, src2, dst, mask):
    from vision.devmat import DeviceMat, _byte_scalar, bitwise
    from vision.utils.helpers import as_mat
    if mask is not None and dst is not None:
        raise error(f"{name}: mask together with dst (cv2 keeps dst's pixels where the mask is 0) is outside the accelerated path")
    a = as_mat(src1)
    b = None if op == _vp.BITWISE_NOT else as_mat(src2)
    mask = None if mask is None else as_mat(mask)
    scalar = 0
    if b is not None and not _is_image(a):
        a, b = b, a                                      # (and, or, xor commute)
    if not _is_image(a):
        raise error(f"{name}: expected an image")
    if b is not None and not _is_image(b):
        scalar, b = _byte_scalar(b), None
        if scalar is None:
            raise error(f"{name}: a scalar operand must be an integer in 0..255 on the accelerated path")
    _check_images(name, *((a,) if b is None else (a, b)))
    if mask is not None:
        if not _is_image(mask) or mask.dtype != np.uint8:
            raise error(f"{name}: the mask must be a uint8 image")
        if mask.ndim == 3 and mask.shape[2] == 1:
            mask = mask.reshaped(mask.shape[:2]) if isinstance(mask, DeviceMat) else mask[:, :, 0]
        if tuple(mask.shape) != tuple(a.shape[:2]):
            raise error(f"{name}: the mask must have the size of the image")
        if a.ndim == 3 and a.shape[2] > 4:
            raise error(f"{name}: at most 4 channels with a mask")
    if any(isinstance(m, DeviceMat) for m in (a, b, mask)):
        return _into(dst, bitwise(op, a, b, scalar, mask))
    r = np.invert(a) if op == _vp.BITWISE_NOT else (np.bitwise_and, np.bitwise_or, np.bitwise_xor)[op](a, np.uint8(scalar) if b is None else b)
    if mask is not None:
        r = np.where((mask if a.ndim == 2 else mask[:, :, None]) != 0, r, np.uint8(0))
    return _into(dst, np.ascontiguousarray(r))


def bitwise_and(src1, src2, dst=None, mask=None):
    """cv2.bitwise_and; where `mask` is 0 the result is 0 (vision_common.py:285 fill_ratio).  With a DeviceMat among the operands:
    libvp vp_bitwise_u8_dev, and the result of two 0/255 masks is known to be one."""
    return _bitwise("bitwise_and", _vp.BITWISE_AND, src1, src2, dst, mask)


def bitwise_or(src1, src2, dst=None, mask=None):
    return _bitwise("bitwise_or", _vp.BITWISE_OR, src1, src2, dst, mask)


def bitwise_xor(src1, src2, dst=None, mask=None):
    return _bitwise("bitwise_xor", _vp.BITWISE_XOR, src1, src2, dst, mask)


def bitwise_not(src, dst=None, mask=None):
    return _bitwise("bitwise_not", _vp.BITWISE_NOT, src, None, dst, mask)


def LUT(src, lut, dst=None):
    """cv2.LUT on uint8 images: one table of 256 uint8 entries for every channel, or one per channel as (256, cn) / (1, 256, cn)."""
    from vision.devmat import DeviceMat
    from vision.utils.helpers import as_mat
    src = as_mat(src)
    if not _is_image(src):
        raise error("LUT: expected an image")
    _check_images("LUT", src)
    lut = np.asarray(as_mat(lut) if not isinstance(lut, DeviceMat) else lut.host(writable=False))
    cn = 1 if src.ndim == 2 else src.shape[2]
    if lut.dtype == np.uint8 and lut.size == 256 and (lut.ndim == 1 or lut.shape in ((256, 1), (1, 256), (1, 256, 1))):
        tables = lut.reshape(1, 256)
    elif lut.dtype == np.uint8 and cn > 1 and lut.shape in ((256, cn), (1, 256, cn)):
        tables = np.ascontiguousarray(lut.reshape(256, cn).T)
    else:
        raise error("LUT: the table must be uint8 with 256 entries, or (256, cn) / (1, 256, cn) for an image of cn channels")
    if isinstance(src, DeviceMat):
        if cn > 4:
            raise error("LUT: at most 4 channels on the accelerated path")
        return _into(dst, _lut_on_device(src, tables))
    if len(tables) == 1:
        return _into(dst, tables[0][src])
    return _into(dst, np.ascontiguousarray(np.stack([tables[c][src[:, :, c]] for c in range(cn)], axis=2)))


def getRotationMatrix2D(center, angle, scale):
    """imgproc/src/imgwarp.cpp getRotationMatrix2D: 2x3 float64 (modules/preprocessor.py:131-133)."""
    return _transform._rotation_matrix_2d(center, angle, scale)


def GaussianBlur(src, ksize, sigmaX, dst=None, sigmaY=0, borderType=None):
    """cv2.GaussianBlur on uint8 images (modules/preprocessor.py:110-114): OpenCV's bit-exact fixed-point path on the GPU.
    Positional order as in cv2: (src, ksize, sigmaX, dst, sigmaY, borderType)."""
    return _into(dst, _transform._gaussian_blur(src, ksize, sigmaX, sigmaY, borderType))


def _source(name, src, dtype_words="only uint8 sources are on the accelerated path"):
    """The packed source of an operator, checked once (vision.utils.helpers.image_source) and refused in the facade's words."""
    return _gather(name, _image_source, _device_source(src)[0],
                   said=(dtype_words, "expected a non-empty (h, w) or (h, w, c) image", "at most 4 channels"))[0]


def medianBlur(src, ksize, dst=None):
    """cv2.medianBlur on uint8 images: the exact order statistic over a replicated border, on the GPU (libvp vp_median_blur_*).
    Positional order as in cv2: (src, ksize, dst).  A DeviceMat stays in HBM (vision.utils.transform.median_blur)."""
    src, _ = _device_source(src)
    try:
        k = int(ksize)
    except (TypeError, ValueError):
        raise error("medianBlur: ksize must be an integer") from None
    if k <= 0 or k % 2 == 0:
        raise error("medianBlur: ksize must be odd and greater than 0")
    if k > 255:
        raise error("medianBlur: ksize above 255 is outside the accelerated path")
    src = _source("medianBlur", src, "only uint8 images are on the accelerated path")
    if src.ndim == 3 and src.shape[2] == 2 and k > 5:
        raise error("medianBlur: 2 channels only with ksize 3 or 5 (cv2 asserts 1, 3 or 4 channels above)")
    return _into(dst, _transform.median_blur(src, k))


# ---- histogram equalisation and CLAHE (libvp vp_clahe.hip) ------------------------------------------------------------------------------
def _grey_u8_source(name, src):
    src, _ = _device_source(src)
    if src.dtype != np.uint8:
        raise error(f"{name}: only uint8 images are on the accelerated path")
    if src.ndim == 3 and src.shape[2] == 1 and isinstance(src, np.ndarray):
        src = src[:, :, 0]
    if src.ndim != 2 or src.size == 0:
        raise error(f"{name}: expected a non-empty single-channel (h, w) image")
    return src


def equalizeHist(src, dst=None):
    """cv2.equalizeHist on a uint8 single-channel image, byte for byte, on the GPU (libvp vp_equalize_hist_*).  A DeviceMat stays in HBM."""
    return _into(dst, _color.equalize_hist(_grey_u8_source("equalizeHist", src)))


class CLAHE:
    """What cv2.createCLAHE returns: apply() runs libvp's vp_clahe_* kernels."""

    def __init__(self, clipLimit=40.0, tileGridSize=(8, 8)):
        self.setClipLimit(clipLimit)
        self.setTilesGridSize(tileGridSize)

    def apply(self, src, dst=None):
        src = _grey_u8_source("CLAHE.apply", src)
        tx, ty = self._grid
        if tx > 64 or ty > 64:
            raise error("CLAHE.apply: more than 64 tiles along an axis is outside the accelerated path")
        try:
            return _into(dst, _gather("CLAHE.apply", _color.clahe, src, self._clip, self._grid))
        except _vp.VpError as e:
            raise error(f"CLAHE.apply: {e}") from None

    def setClipLimit(self, clipLimit):
        try:
            clip = float(clipLimit)
        except (TypeError, ValueError):
            raise error("CLAHE: clipLimit must be a number") from None
        if clip != clip:
            raise error("CLAHE: clipLimit must not be NaN")
        self._clip = clip

    def getClipLimit(self):
        return self._clip

    def setTilesGridSize(self, tileGridSize):
        try:
            tx, ty = (int(v) for v in tileGridSize)
        except (TypeError, ValueError):
            raise error("CLAHE: tileGridSize must be a pair of integers") from None
        if tx < 1 or ty < 1:
            raise error("CLAHE: tileGridSize must be at least (1, 1)")
        self._grid = (tx, ty)

    def getTilesGridSize(self):
        return self._grid

    def collectGarbage(self):
        """cv2 frees its cached tables here; this object keeps none."""


def createCLAHE(clipLimit=40.0, tileGridSize=(8, 8)):
    """cv2.createCLAHE: contrast-limited adaptive histogram equalisation of uint8 single-channel images, byte for byte OpenCV's result
    (DESIGN.md section 4), on the GPU.  apply() of a DeviceMat stays in HBM."""
    return CLAHE(clipLimit, tileGridSize)


# ---- stereo block matching (libvp vp_stereo.hip) ---------------------------------------------------------------
StereoBM_PREFILTER_NORMALIZED_RESPONSE, StereoBM_PREFILTER_XSOBEL = 0, 1
STEREO_BM_PREFILTER_NORMALIZED_RESPONSE, STEREO_BM_PREFILTER_XSOBEL = 0, 1


class StereoBM:
    """What cv2.StereoBM_create returns: compute() runs libvp's vp_stereo_bm_* kernels on the statement of tests/stereo_restate.py
    (vision.utils.stereo.disparity).  Six parameters are supported; the prefilter is always XSOBEL; the speckle filter, the left-right
    check, the ROIs and preFilterSize keep cv2's defaults and any other value is refused."""
    # name -> (default, getter / setter suffix) of what this path does not have
    _FIXED = {"SpeckleWindowSize": 0, "SpeckleRange": 0, "Disp12MaxDiff": -1, "PreFilterType": StereoBM_PREFILTER_XSOBEL, "PreFilterSize": 9,
              "ROI1": (0, 0, 0, 0), "ROI2": (0, 0, 0, 0)}
    _KEYS = {"NumDisparities": "num_disparities", "BlockSize": "block_size", "MinDisparity": "min_disparity", "PreFilterCap": "pre_filter_cap",
             "TextureThreshold": "texture_threshold", "UniquenessRatio": "uniqueness_ratio"}

    def __init__(self, numDisparities=0, blockSize=21):
        self._p = dict(num_disparities=64, block_size=21, min_disparity=0, pre_filter_cap=31, texture_threshold=10, uniqueness_ratio=15)
        self.setNumDisparities(numDisparities)
        self.setBlockSize(blockSize)

    def _set(self, key, value):
        from vision.utils import stereo as _stereo
        trial = dict(self._p, **{key: value})
        _gather("StereoBM", _stereo._matcher, **trial)
        self._p = trial

    def setNumDisparities(self, numDisparities):
        self._set("num_disparities", 64 if numDisparities == 0 else numDisparities)

    def compute(self, left, right, disparity=None):
        from vision.utils import stereo as _stereo
        left, right = _grey_u8_source("StereoBM.compute", left), _grey_u8_source("StereoBM.compute", right)
        try:
            return _into(disparity, _gather("StereoBM.compute", _stereo.disparity, left, right, **self._p))
        except _vp.VpError as e:
            raise error(f"StereoBM.compute: {e}") from None


def _stereo_bm_accessors():
    for name, key in StereoBM._KEYS.items():
        setattr(StereoBM, "get" + name, lambda self, key=key: self._p[key])
        if name != "NumDisparities":
            setattr(StereoBM, "set" + name, lambda self, value, key=key: self._set(key, value))
    for name, default in StereoBM._FIXED.items():
        def setter(self, value, name=name, default=default):
            if (tuple(value) if isinstance(default, tuple) else value) != default:
                raise error(f"StereoBM: {name} other than {default} is outside the accelerated path (DESIGN.md section 7)")
        setattr(StereoBM, "get" + name, lambda self, default=default: default)
        setattr(StereoBM, "set" + name, setter)


_stereo_bm_accessors()


def StereoBM_create(numDisparities=0, blockSize=21):
    """cv2.StereoBM_create: block matching of a rectified uint8 pair on the GPU; numDisparities 0 means 64.  compute(left, right) gives
    16 times the disparity as int16 ((minDisparity - 1) * 16 where there is no answer); DeviceMat images give a DeviceMat."""
    return StereoBM(numDisparities, blockSize)


StereoBM.create = staticmethod(StereoBM_create)


def filterSpeckles(img, newVal, maxSpeckleSize, maxDiff, buf=None):
    """cv2.filterSpeckles on a 2-D int16 disparity image, in place, on the GPU (libvp vp_filter_speckles_*; the rule is
    tests/speckle_restate.py's): regions of at most maxSpeckleSize pixels become newVal.  Returns (img, buf) as
    cv2 does; buf is not used.  A DeviceMat that lives in HBM is filtered there."""
    from vision.devmat import DeviceMat
    from vision.utils import stereo as _stereo
    if not isinstance(img, (np.ndarray, DeviceMat)) or img.dtype != np.int16 or img.ndim != 2 or img.size == 0:
        raise error("filterSpeckles: only non-empty 2-D int16 images are on the accelerated path")
    try:
        params = _stereo._speckle_args(img, maxSpeckleSize, maxDiff, newVal)
        ctx = _vp.default_context()
        if isinstance(img, DeviceMat) and img._host is None and img.device_valid_for(ctx):
            img.dev_ptr                                  # a pending result is computed first
            img._before_write()
            _stereo._speckles_dev(ctx, img, params, out=img)
            return img, buf
        host = img.host(writable=True, escape=False) if isinstance(img, DeviceMat) else img
        if not host.flags.writeable:
            raise error("filterSpeckles: the image is read-only")
        packed = host if host.flags.c_contiguous else np.ascontiguousarray(host)
        h, w = packed.shape
        _vp.check(_vp.lib().vp_filter_speckles_i16(ctx.handle, packed.ctypes.data, w, h, *params, packed.ctypes.data), ctx.handle)
        if packed is not host:
            host[...] = packed
        return img, buf
    except (TypeError, ValueError, _vp.VpError) as e:
        raise error(f"filterSpeckles: {e}") from None


# ---- stereo rectification and reprojection (libvp vp_rectify.hip) ---------------------------------------------
CALIB_ZERO_DISPARITY = 1024


def stereoRectify(cameraMatrix1, distCoeffs1, cameraMatrix2, distCoeffs2, imageSize, R, T, R1=None, R2=None, P1=None, P2=None, Q=None,
                  flags=CALIB_ZERO_DISPARITY, alpha=-1, newImageSize=(0, 0)):
    """cv2.stereoRectify: (R1, R2, P1, P2, Q, validPixROI1, validPixROI2) by Bouguet's algorithm, host numpy in float64
    (vision.utils.stereo.stereo_rectify has the steps); run once per calibration.  The statement is this library's own: cv2's bits
    are not claimed.  flags: 0 or CALIB_ZERO_DISPARITY; newImageSize (0, 0) means imageSize.  The maps come from
    initUndistortRectifyMap with R1 / P1 and R2 / P2; vision.utils.stereo.StereoRig keeps them in HBM."""
    from vision.utils import stereo as _stereo
    if flags not in (0, CALIB_ZERO_DISPARITY):
        raise error("stereoRectify: flags must be 0 or CALIB_ZERO_DISPARITY")
    new_size = None if newImageSize is None or tuple(newImageSize) == (0, 0) else newImageSize
    out = _gather("stereoRectify", _stereo.stereo_rectify, cameraMatrix1, distCoeffs1, cameraMatrix2, distCoeffs2, imageSize, R, T,
                  flags == CALIB_ZERO_DISPARITY, alpha, new_size)
    for given, made in zip((R1, R2, P1, P2, Q), out):
        if given is not None:
            _into(given, made)
    return out


def reprojectImageTo3D(disparity, Q, _3dImage=None, handleMissingValues=False, ddepth=-1):
    """cv2.reprojectImageTo3D on the GPU (libvp vp_reproject_to_3d_*): float32 (h, w, 3) points of an int16 or float32 (h, w) disparity
    image, (X / W, Y / W, Z / W) of Q (x, y, d, 1) in double.  As in cv2 the values of the image are the disparities as they stand: a
    matcher's int16 result, 16 times the disparity, is divided by 16 by the caller (vision.utils.stereo.reproject_to_3d and
    StereoRig.points take it as it is).  Pixels with W == 0 or a disparity that is not finite give three zeros.
    handleMissingValues=True is refused: cv2's 10000-Z mark is not this library's zero convention.  ddepth: -1 or CV_32F."""
    from vision.devmat import DeviceMat
    from vision.utils import stereo as _stereo
    if handleMissingValues:
        raise error("reprojectImageTo3D: handleMissingValues marks pixels with Z = 10000; this library marks them with zeros (DESIGN.md section 7)")
    if ddepth not in (-1, CV_32F):
        raise error("reprojectImageTo3D: ddepth must be -1 or CV_32F")
    disp = _as(disparity)
    if isinstance(disp, (np.ndarray, DeviceMat)) and disp.ndim == 3 and disp.shape[2] == 1:
        disp = disp.reshaped(disp.shape[:2]) if isinstance(disp, DeviceMat) else disp[:, :, 0]
    if isinstance(disp, np.ndarray) and disp.dtype == np.int16:
        disp = disp.astype(np.float32)                    # cv2 reads the int16 values as pixels; every int16 is exact in float32
    elif isinstance(disp, DeviceMat) and disp.dtype == np.int16:
        raise error("reprojectImageTo3D: an int16 image in HBM holds sixteenths of a pixel: vision.utils.stereo.reproject_to_3d reads it as such")
    try:
        return _into(_3dImage, _gather("reprojectImageTo3D", _stereo.reproject_to_3d, disp, Q))
    except _vp.VpError as e:
        raise error(f"reprojectImageTo3D: {e}") from None


# ---- derivative filters (libvp vp_deriv.hip) ------------------------------------------------------------------------------------------
def _deriv_call(name, fn, src, ddepth, scale, delta, borderType, *args):
    """What cv2 rejects, and the two restrictions of this path: scale = 1 and delta = 0 only."""
    src = _source(name, src)
    if scale != 1 or delta != 0:
        raise error(f"{name}: scale != 1 or delta != 0 takes OpenCV's float paths, which this library does not restate (DESIGN.md section 7)")
    return _gather(name, fn, src, *args, ddepth, BORDER_DEFAULT if borderType is None else borderType)


def Sobel(src, ddepth, dx, dy, dst=None, ksize=3, scale=1, delta=0, borderType=BORDER_DEFAULT):
    """cv2.Sobel on uint8 images with scale = 1 and delta = 0, on the GPU: the exact integer correlation, cast to ddepth (-1 / CV_8U,
    CV_16S, CV_32F, CV_64F) as saturate_cast does.  Positional order as in cv2.  A DeviceMat stays in HBM and comes back with the
    requested dtype."""
    return _into(dst, _deriv_call("Sobel", _transform.sobel, src, ddepth, scale, delta, borderType, dx, dy, ksize))


def Scharr(src, ddepth, dx, dy, dst=None, scale=1, delta=0, borderType=BORDER_DEFAULT):
    """cv2.Scharr under the rules of Sobel above: [-1 0 1] with [3 10 3], dx + dy == 1."""
    return _into(dst, _deriv_call("Scharr", _transform.scharr, src, ddepth, scale, delta, borderType, dx, dy))


def Laplacian(src, ddepth, dst=None, ksize=1, scale=1, delta=0, borderType=BORDER_DEFAULT):
    """cv2.Laplacian under the rules of Sobel above: ksize 1, 3 (the 3x3 kernels), 5 or 7 (Sobel(2, 0) + Sobel(0, 2))."""
    return _into(dst, _deriv_call("Laplacian", _transform.laplacian, src, ddepth, scale, delta, borderType, ksize))


def spatialGradient(src, dx=None, dy=None, ksize=3, borderType=BORDER_DEFAULT):
    """cv2.spatialGradient: (dx, dy) = (Sobel(1, 0, 3), Sobel(0, 1, 3)) as int16 from one pass over a single-channel uint8 image;
    ksize 3 and BORDER_DEFAULT or BORDER_REPLICATE only, as cv2."""
    src, _ = _device_source(src)
    if src.dtype != np.uint8:
        raise error("spatialGradient: only uint8 sources")
    gx, gy = _gather("spatialGradient", _transform.spatial_gradient, src, ksize, BORDER_DEFAULT if borderType is None else borderType)
    return _into(dx, gx), _into(dy, gy)


def convertScaleAbs(src, dst=None, alpha=1, beta=0):
    """cv2.convertScaleAbs with alpha = 1 and beta = 0: saturate_cast<uchar>(|v|) of a uint8, int16, float32 or float64 image, on the
    GPU; a device image (the int16 result of Sobel) gives a device uint8 image.  Other alpha / beta: DESIGN.md section 7."""
    if alpha != 1 or beta != 0:
        raise error("convertScaleAbs: alpha != 1 or beta != 0 is outside the accelerated path (DESIGN.md section 7)")
    src, _ = _device_source(src)
    return _into(dst, _gather("convertScaleAbs", _transform.convert_scale_abs, src))


# ---- box filter, pyramid steps, integral image (libvp vp_box.hip, vp_pyr.hip, vp_integral.hip) ------------------------------------------
def _ksize(name, ksize, anchor):
    try:
        kw, kh = (int(v) for v in ksize)
    except (TypeError, ValueError):
        raise error(f"{name}: ksize must be a pair of integers") from None
    if kw < 1 or kh < 1:
        raise error(f"{name}: ksize must be positive")
    a = (-1, -1) if anchor is None else tuple(int(v) for v in anchor)
    if a not in ((-1, -1), (kw // 2, kh // 2)):
        raise error(f"{name}: only the default anchor (the window's centre) is on the accelerated path")
    return kw, kh


def boxFilter(src, ddepth, ksize, dst=None, anchor=(-1, -1), normalize=True, borderType=BORDER_DEFAULT):
    """cv2.boxFilter on uint8 images, on the GPU, pure integer arithmetic: unnormalised sums cast to ddepth (-1 / CV_8U, CV_16S, CV_32S,
    CV_32F, CV_64F); normalised, CV_8U only and only window areas on which OpenCV's own roundings agree.
    Positional order as in cv2.  A DeviceMat stays in HBM."""
    src = _source("boxFilter", src)
    kw, kh = _ksize("boxFilter", ksize, anchor)
    return _into(dst, _gather("boxFilter", _transform.box_filter, src, kw, kh, ddepth, normalize, BORDER_DEFAULT if borderType is None else borderType))


def blur(src, ksize, dst=None, anchor=(-1, -1), borderType=BORDER_DEFAULT):
    """cv2.blur: the normalised box filter (see boxFilter)."""
    src = _source("blur", src)
    kw, kh = _ksize("blur", ksize, anchor)
    return _into(dst, _gather("blur", _transform.box_filter, src, kw, kh, -1, True, BORDER_DEFAULT if borderType is None else borderType))


def _default_dstsize(name, dstsize, want):
    if dstsize is not None and tuple(int(v) for v in dstsize) not in ((0, 0), want):
        raise error(f"{name}: only the default dstsize {want} is on the accelerated path")


def pyrDown(src, dst=None, dstsize=None, borderType=BORDER_DEFAULT):
    """cv2.pyrDown on uint8 images, on the GPU: ((w + 1) // 2, (h + 1) // 2); BORDER_DEFAULT, BORDER_REPLICATE or BORDER_REFLECT."""
    src = _source("pyrDown", src)
    _default_dstsize("pyrDown", dstsize, ((src.shape[1] + 1) // 2, (src.shape[0] + 1) // 2))
    return _into(dst, _gather("pyrDown", _transform.pyr_down, src, BORDER_DEFAULT if borderType is None else borderType))


def pyrUp(src, dst=None, dstsize=None, borderType=BORDER_DEFAULT):
    """cv2.pyrUp on uint8 images, on the GPU: (2w, 2h); BORDER_DEFAULT only, as cv2."""
    src = _source("pyrUp", src)
    _default_dstsize("pyrUp", dstsize, (2 * src.shape[1], 2 * src.shape[0]))
    return _into(dst, _gather("pyrUp", _transform.pyr_up, src, BORDER_DEFAULT if borderType is None else borderType))


def buildPyramid(src, maxlevel):
    """cv2.buildPyramid: the list [src, pyrDown(src), ...] of maxlevel + 1 images; a DeviceMat's levels never visit the host."""
    src = _source("buildPyramid", src)
    return _gather("buildPyramid", _transform.build_pyramid, src, maxlevel)


def integral(src, sum=None, sdepth=-1):
    """cv2.integral on uint8 images, on the GPU: (h + 1, w + 1[, cn]) int32; sdepth -1 or CV_32S."""
    if sdepth not in (-1, CV_32S):
        raise error("integral: only sdepth -1 / CV_32S is on the accelerated path")
    src = _source("integral", src)
    return _into(sum, _gather("integral", _transform.integral, src))


def integral2(*args, **kwargs):
    raise error("integral2: the squared sums are outside the accelerated path (DESIGN.md section 7)")


def integral3(*args, **kwargs):
    raise error("integral3: the squared and tilted sums are outside the accelerated path (DESIGN.md section 7)")


INTER_LINEAR = 1
WARP_INVERSE_MAP = 16


def warpAffine(src, M, dsize, dst=None, flags=INTER_LINEAR, borderMode=BORDER_CONSTANT, borderValue=0):
    """cv2.warpAffine with bilinear interpolation on uint8 images (modules/preprocessor.py:130-135,145-149): OpenCV's classical
    fixed-point path on the GPU (libvp vp_warp_affine_u8).  Positional order as in cv2: (src, M, dsize, dst, flags, borderMode,
    borderValue)."""
    return _into(dst, _transform._warp_affine(src, M, dsize, flags, borderMode, borderValue))


INTER_NEAREST = 0
CV_16UC1, CV_32FC1, CV_16SC2, CV_32FC2 = 2, 5, 11, 13


def remap(src, map1, map2, interpolation, dst=None, borderMode=BORDER_CONSTANT, borderValue=0):
    """cv2.remap on uint8 images of 1..4 channels, INTER_LINEAR or INTER_NEAREST, BORDER_CONSTANT or BORDER_REPLICATE: OpenCV's
    classical fixed-point path byte for byte, on the GPU (libvp vp_remap_*).  Maps (numpy or DeviceMat): two
    float32 planes; one float32 (h, w, 2) plane with map2 None or empty; convertMaps' fixed form (int16 (h, w, 2) + uint16 (h, w));
    or, with INTER_NEAREST, an int16 (h, w, 2) plane alone.  A DeviceMat in gives a DeviceMat out, numpy gives numpy."""
    if interpolation not in (INTER_NEAREST, INTER_LINEAR):
        raise error("remap: only INTER_NEAREST and INTER_LINEAR are on the accelerated path")
    if borderMode not in (BORDER_CONSTANT, BORDER_REPLICATE):
        raise error("remap: only BORDER_CONSTANT and BORDER_REPLICATE are on the accelerated path")
    src, _ = _device_source(src)
    return _into(dst, _gather("remap", _transform._remap, src, map1, map2, interpolation == INTER_NEAREST, borderMode, borderValue))


def warpPerspective(src, M, dsize, dst=None, flags=INTER_LINEAR, borderMode=BORDER_CONSTANT, borderValue=0):
    """cv2.warpPerspective on uint8 images of 1..4 channels; flags: INTER_LINEAR or INTER_NEAREST, optionally | WARP_INVERSE_MAP.
    OpenCV's classical fixed-point path byte for byte, on the GPU (libvp vp_warp_perspective_*)."""
    if flags is None:
        flags = INTER_LINEAR
    if (flags & ~WARP_INVERSE_MAP) not in (INTER_NEAREST, INTER_LINEAR):
        raise error("warpPerspective: only INTER_NEAREST and INTER_LINEAR are on the accelerated path")
    if borderMode not in (BORDER_CONSTANT, BORDER_REPLICATE):
        raise error("warpPerspective: only BORDER_CONSTANT and BORDER_REPLICATE are on the accelerated path")
    src, _ = _device_source(src)
    try:
        dw, dh = int(dsize[0]), int(dsize[1])
    except (TypeError, ValueError, IndexError):
        raise error("warpPerspective: dsize must be (width, height)") from None
    return _into(dst, _gather("warpPerspective", _transform._warp_perspective, src, M, dw, dh, bool(flags & WARP_INVERSE_MAP),
                              (flags & ~WARP_INVERSE_MAP) == INTER_NEAREST, borderMode, borderValue))


def convertMaps(map1, map2, dstmap1type, nninterpolation=False):
    """cv2.convertMaps from float32 maps (two planes, or one (h, w, 2) plane with map2 None or empty) to the fixed form:
    (int16 (h, w, 2), uint16 (h, w)), or (int16 (h, w, 2) of rounded coordinates, empty) with nninterpolation.  On the GPU (libvp
    vp_convert_maps_dev), byte for byte; DeviceMat maps give DeviceMat maps.  The other directions are outside the path."""
    from vision.devmat import DeviceMat
    if dstmap1type != CV_16SC2:
        raise error("convertMaps: only the conversion to CV_16SC2 is on the accelerated path")
    kind = _gather("convertMaps", _transform._classify_maps, map1, map2)[0]
    if kind == "fixed":
        raise error("convertMaps: only float32 source maps are on the accelerated path")
    on_dev = any(isinstance(_as(m), DeviceMat) for m in (map1, map2) if m is not None)
    t = _gather("convertMaps", _transform.RemapTable, map1, map2, bool(nninterpolation))
    if on_dev:
        return t.xy, (np.empty((0,), np.uint16) if t.frac is None else t.frac)
    return t.xy.host_copy(), (np.empty((0,), np.uint16) if t.frac is None else t.frac.host_copy())


def _as(m):
    from vision.utils.helpers import as_mat
    return as_mat(m)


def initUndistortRectifyMap(cameraMatrix, distCoeffs, R, newCameraMatrix, size, m1type):
    """cv2.initUndistortRectifyMap for the rational model without thin-prism and tilt terms (4, 5 or 8 coefficients), host numpy in
    float64: run once per calibration.  m1type CV_32FC1 -> (mapx, mapy), CV_32FC2 -> (interleaved map, empty), CV_16SC2 -> the fixed
    form.  Within an ulp of float32 of cv2's maps, not bit for bit."""
    if m1type not in (CV_32FC1, CV_32FC2, CV_16SC2):
        raise error("initUndistortRectifyMap: m1type must be CV_32FC1, CV_32FC2 or CV_16SC2")
    u, v = _transform._undistort_coords("initUndistortRectifyMap", cameraMatrix, distCoeffs, R, newCameraMatrix, size)
    if m1type == CV_32FC1:
        return u.astype(np.float32), v.astype(np.float32)
    if m1type == CV_32FC2:
        return np.ascontiguousarray(np.stack([u, v], axis=-1).astype(np.float32)), np.empty((0,), np.float32)
    return _transform._fixed_from_double(u, v)


def undistort(src, cameraMatrix, distCoeffs, dst=None, newCameraMatrix=None):
    """cv2.undistort: initUndistortRectifyMap(R = identity, CV_16SC2) of the image's size, then remap(INTER_LINEAR,
    BORDER_CONSTANT 0) on the GPU.  For a stream of frames build the table once: vision.utils.transform.undistorter."""
    src, _ = _transform._plain_source("undistort", src, "expected a non-empty uint8 image")
    xy, frac = initUndistortRectifyMap(cameraMatrix, distCoeffs, None, newCameraMatrix, (src.shape[1], src.shape[0]), CV_16SC2)
    return _into(dst, _gather("undistort", _transform._remap, src, xy, frac, False, BORDER_CONSTANT, 0))


def getPerspectiveTransform(src, dst, solveMethod=0):
    """cv2.getPerspectiveTransform: the 3x3 float64 matrix (M[2, 2] = 1) that maps four source points to four destination points;
    the 8x8 system solved in float64 on the host.  Not claimed bit-exact."""
    s = np.asarray(src, dtype=np.float64).reshape(-1, 2)
    d = np.asarray(dst, dtype=np.float64).reshape(-1, 2)
    if s.shape != (4, 2) or d.shape != (4, 2):
        raise error("getPerspectiveTransform: four source and four destination points")
    a = np.zeros((8, 8))
    b = np.zeros(8)
    for i in range(4):
        a[i] = [s[i, 0], s[i, 1], 1, 0, 0, 0, -s[i, 0] * d[i, 0], -s[i, 1] * d[i, 0]]
        a[i + 4] = [0, 0, 0, s[i, 0], s[i, 1], 1, -s[i, 0] * d[i, 1], -s[i, 1] * d[i, 1]]
        b[i], b[i + 4] = d[i, 0], d[i, 1]
    try:
        x = np.linalg.solve(a, b)
    except np.linalg.LinAlgError:
        raise error("getPerspectiveTransform: the points are degenerate") from None
    return np.append(x, 1.0).reshape(3, 3)


def perspectiveTransform(src, m, dst=None):
    """cv2.perspectiveTransform of 2-D points ((N, 1, 2) or (N, 2), float32 or float64) by a 3x3 matrix, host numpy in float64:
    (x', y') = (m00 x + m01 y + m02, m10 x + m11 y + m12) / w with w = m20 x + m21 y + m22; 0 where w is 0."""
    p = np.asarray(src)
    M = np.asarray(m, dtype=np.float64)
    if p.dtype not in (np.float32, np.float64) or p.ndim not in (2, 3) or p.shape[-1] != 2 or M.shape != (3, 3):
        raise error("perspectiveTransform: float32 / float64 points of 2 channels and a 3x3 matrix")
    x, y = p[..., 0].astype(np.float64), p[..., 1].astype(np.float64)
    w = M[2, 0] * x + M[2, 1] * y + M[2, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(w != 0, 1.0 / w, 0.0)
    out = np.stack([(M[0, 0] * x + M[0, 1] * y + M[0, 2]) * w, (M[1, 0] * x + M[1, 1] * y + M[1, 2]) * w], axis=-1).astype(p.dtype)
    return _into(dst, out)


def resize(src, dsize, dst=None, fx=None, fy=None, interpolation=INTER_LINEAR):
    """cv2.resize(src, (width, height)) with the default bilinear interpolation, uint8 images (modules/preprocessor.py:136-144).
    Positional order as in cv2: (src, dsize, dst, fx, fy, interpolation); dsize None or (0, 0) takes the size from fx / fy."""
    return _into(dst, _transform._resize(src, dsize, fx, fy, interpolation))


def Canny(image, threshold1, threshold2, apertureSize=3, L2gradient=False):
    """cv2.Canny on uint8 images with the defaults the reference uses (utils/feature.py:66,101): 3x3 Sobel, L1 gradient magnitude."""
    from vision import _vp
    if apertureSize != 3 or L2gradient:
        raise error("Canny: only apertureSize=3 with the L1 gradient is on the accelerated path")
    image = np.ascontiguousarray(image)
    if image.dtype != np.uint8 or image.ndim not in (2, 3) or image.size == 0:
        raise error("Canny: expected a non-empty uint8 image")
    cn = 1 if image.ndim == 2 else image.shape[2]
    if cn > 4:
        raise error("Canny: at most 4 channels")
    out = np.empty(image.shape[:2], np.uint8)
    ctx = _vp.default_context()
    _vp.check(_vp.lib().vp_canny_u8(ctx.handle, _vp.ptr(image), image.shape[1], image.shape[0], cn, float(threshold1), float(threshold2),
                                    _vp.ptr(out)), ctx.handle)
    return out


def HoughLines(image, rho, theta, threshold, lines=None, srn=0, stn=0, min_theta=0, max_theta=CV_PI):
    """cv2.HoughLines (utils/feature.py:209) in cv2's positional order: (N, 1, 2) float32 (rho, theta), or None when nothing is found.
    The multi-scale variant (srn or stn non-zero) is outside the accelerated path."""
    if srn or stn:
        raise error("HoughLines: the multi-scale transform (srn / stn != 0) is outside the accelerated path")
    if not (rho > 0 and theta > 0):
        raise error("HoughLines: rho and theta must be positive")
    if max_theta < min_theta:
        raise error("HoughLines: max_theta must be greater than min_theta")
    return _feature.hough_lines(image, rho, theta, threshold, min_theta, max_theta)


def HoughCircles(image, method, dp, minDist, circles=None, param1=100, param2=100, minRadius=0, maxRadius=0):
    """cv2.HoughCircles (utils/feature.py:128-155) in cv2's positional order: (1, N, 3) float32 (x, y, r), or None when nothing is found.
    HOUGH_GRADIENT only; HOUGH_GRADIENT_ALT and the centres-only mode (maxRadius < 0) are outside the accelerated path."""
    from vision.devmat import DeviceMat
    if method == HOUGH_GRADIENT_ALT:
        raise error("HoughCircles: HOUGH_GRADIENT_ALT is outside the accelerated path")
    if method != HOUGH_GRADIENT:
        raise error("HoughCircles: unknown method")
    if maxRadius < 0:
        raise error("HoughCircles: the centres-only mode (maxRadius < 0) is outside the accelerated path")
    if not (dp > 0 and minDist > 0 and param1 > 0 and param2 > 0):
        raise error("HoughCircles: dp, minDist, param1 and param2 must be positive")
    shape = tuple(image.shape) if isinstance(image, (np.ndarray, DeviceMat)) else ()
    if (not isinstance(image, (np.ndarray, DeviceMat)) or image.dtype != np.uint8 or len(shape) not in (2, 3) or (len(shape) == 3 and shape[2] != 1)
            or shape[0] == 0 or shape[1] == 0):
        raise error("HoughCircles: the image must be a non-empty CV_8UC1 image")
    try:
        return _feature.hough_circles(image, dp, minDist, param1, param2, minRadius, maxRadius)
    except _vp.VpError as e:
        raise error(f"HoughCircles: {e}") from e


# ---- corners (libvp vp_corners.hip): the exact value of what OpenCV's float32 code approximates, DESIGN.md section 4.24 ----------------
def cornerMinEigenVal(src, blockSize, dst=None, ksize=3, borderType=BORDER_DEFAULT):
    """cv2.cornerMinEigenVal on a uint8 single-channel image in cv2's positional order: float32 (h, w), the smaller eigenvalue of the
    structure tensor from exact integer sums (ksize 3 only; blockSize 1..31).  A DeviceMat stays in HBM."""
    src = _source("cornerMinEigenVal", src, "only uint8 images are on the accelerated path")
    return _into(dst, _gather("cornerMinEigenVal", _feature.corner_min_eigen_val, src, blockSize, ksize, BORDER_DEFAULT if borderType is None else borderType))


def cornerHarris(src, blockSize, ksize, k, dst=None, borderType=BORDER_DEFAULT):
    """cv2.cornerHarris under the rules of cornerMinEigenVal above: det - k trace^2 of the same structure tensor."""
    src = _source("cornerHarris", src, "only uint8 images are on the accelerated path")
    return _into(dst, _gather("cornerHarris", _feature.corner_harris, src, blockSize, ksize, k, BORDER_DEFAULT if borderType is None else borderType))


def goodFeaturesToTrack(image, maxCorners, qualityLevel, minDistance, corners=None, mask=None, blockSize=3, useHarrisDetector=False, k=0.04,
                        gradientSize=3):
    """cv2.goodFeaturesToTrack (utils/feature.py `find_corners`) in cv2's positional order on a uint8 single-channel image: float32
    (N, 1, 2) of (x, y), strongest first, or None when there is no corner.  gradientSize 3 only."""
    if gradientSize != 3:
        raise error("goodFeaturesToTrack: only gradientSize 3 is on the accelerated path (DESIGN.md section 7)")
    image = _source("goodFeaturesToTrack", image, "only uint8 images are on the accelerated path")
    try:
        found = _gather("goodFeaturesToTrack", _feature.good_features_to_track, image, maxCorners, qualityLevel, minDistance, mask, blockSize,
                        useHarrisDetector, k)
    except _vp.VpError as e:
        raise error(f"goodFeaturesToTrack: {e}") from e
    return found if found is None else _into(corners, found)


# ---- distances (libvp vp_dist.hip): exact L2, L1 and C distances to the nearest zero pixel, DESIGN.md section 4.25 -------------------------
DIST_USER, DIST_L1, DIST_L2, DIST_C, DIST_L12, DIST_FAIR, DIST_WELSCH, DIST_HUBER = -1, 1, 2, 3, 4, 5, 6, 7
DIST_MASK_3, DIST_MASK_5, DIST_MASK_PRECISE = 3, 5, 0


def distanceTransform(src, distanceType, maskSize, dst=None, dstType=CV_32F):
    """cv2.distanceTransform on a uint8 single-channel image in cv2's positional order.  DIST_L2 with DIST_MASK_PRECISE: the correctly
    rounded float32 root of the exact squared distance; DIST_L1 and DIST_C with any mask size (cv2 forces 3): exact integers, DIST_L1
    also as CV_8U.  DIST_L2 with a 3x3 or 5x5 mask is cv2's chamfer approximation, which is not restated.  An
    image without a zero pixel gives +inf (255) everywhere.  A DeviceMat stays in HBM (vision.utils.feature.distance_transform)."""
    if distanceType not in (DIST_L1, DIST_L2, DIST_C):
        raise error("distanceTransform: only DIST_L1, DIST_L2 and DIST_C are on the accelerated path")
    if maskSize not in (DIST_MASK_3, DIST_MASK_5, DIST_MASK_PRECISE):
        raise error("distanceTransform: maskSize must be DIST_MASK_3, DIST_MASK_5 or DIST_MASK_PRECISE")
    if distanceType == DIST_L2 and maskSize != DIST_MASK_PRECISE:
        raise error("distanceTransform: DIST_L2 only with DIST_MASK_PRECISE - the 3x3 and 5x5 chamfer approximations are not restated "
                    "(DESIGN.md section 7)")
    if dstType not in (CV_8U, CV_32F):
        raise error("distanceTransform: dstType must be CV_8U or CV_32F")
    src = _source("distanceTransform", src, "only uint8 images are on the accelerated path")
    return _into(dst, _gather("distanceTransform", _feature.distance_transform, src, distanceType, np.uint8 if dstType == CV_8U else np.float32))


def minMaxLoc(src, mask=None):
    """cv2.minMaxLoc on a uint8 or float32 single-channel image: (minVal, maxVal, minLoc, maxLoc), ties to the first pixel in raster
    order.  NaN pixels take no part; an empty mask gives (0.0, 0.0, (-1, -1), (-1, -1))."""
    return _gather("minMaxLoc", _feature.min_max_loc, _device_source(src)[0], mask)


# ---- template matching (libvp vp_match.hip): the exact value of what cv2.matchTemplate approximates, DESIGN.md section 4.27 -------------
TM_SQDIFF, TM_SQDIFF_NORMED, TM_CCORR, TM_CCORR_NORMED, TM_CCOEFF, TM_CCOEFF_NORMED = 0, 1, 2, 3, 4, 5


def matchTemplate(image, templ, method, result=None, mask=None):
    """cv2.matchTemplate on uint8 images of 1..4 channels in cv2's positional order: the float32 map of (H - h + 1, W - w + 1) scores.
    The sums under a score are exact integers and the steps after them cv2's in double arithmetic; cv2's own values differ from these
    by the error of its float32 DFT.  mask=, float32 images, templates above 65536 bytes and a template larger than the image are
    refused.  A DeviceMat image stays in HBM (vision.utils.feature.match_template)."""
    if mask is not None:
        raise error("matchTemplate: mask= is not on the accelerated path")
    if method not in (TM_SQDIFF, TM_SQDIFF_NORMED, TM_CCORR, TM_CCORR_NORMED, TM_CCOEFF, TM_CCOEFF_NORMED):
        raise error("matchTemplate: the method must be one of the six TM_* values")
    image = _source("matchTemplate", image, "only uint8 images are on the accelerated path")
    if not isinstance(templ, _feature.DeviceCrop):
        templ = _source("matchTemplate", templ, "only uint8 templates are on the accelerated path")
    return _into(result, _gather("matchTemplate", _feature.match_template, image, templ, method))


# ---- k-means (libvp vp_kmeans.hip): the exact value of what cv2.kmeans approximates, DESIGN.md section 4.26 -------------------------------
KMEANS_RANDOM_CENTERS, KMEANS_USE_INITIAL_LABELS, KMEANS_PP_CENTERS = 0, 1, 2
TERM_CRITERIA_COUNT = TERM_CRITERIA_MAX_ITER = 1
TERM_CRITERIA_EPS = 2
_FLT_EPSILON = 1.1920928955078125e-07


def _kmeans_image_shape(n):
    """(h, w), both at most 4096, with h w == n: the samples are clustered as the pixels of such an image (the raster order, and with
    it every result, is the same for every such shape); None when n has no such pair of factors"""
    for w in range(min(n, 4096), 0, -1):
        if n % w == 0:
            return (n // w, w) if n // w <= 4096 else None
    return None


def kmeans(data, K, bestLabels, criteria, attempts, flags, centers=None):
    """cv2.kmeans in cv2's positional order on (N, d) samples, d <= 4, uint8 or float32 holding integers in 0..255 (the pixels of an
    image, `img.reshape(-1, 3)`), N <= 2^24 with N = h w for some h, w <= 4096: (compactness, labels (N, 1) int32, centers (K, d)
    float32), computed on the GPU as DESIGN.md section 4.26 states it (vision.utils.color.kmeans).  criteria is read as OpenCV reads
    it: without the COUNT bit 100 iterations, with it maxCount clamped to 2..100; without the EPS bit eps = FLT_EPSILON.
    KMEANS_RANDOM_CENTERS starts every attempt a from K distinct samples drawn from np.random.default_rng(a) - OpenCV draws K points
    uniformly in the bounding box of the data from cv::theRNG(), which no restatement can follow -, and the attempt with the smallest
    compactness wins.  KMEANS_PP_CENTERS and KMEANS_USE_INITIAL_LABELS are outside the accelerated path."""
    if flags != KMEANS_RANDOM_CENTERS:
        raise error("kmeans: only KMEANS_RANDOM_CENTERS is on the accelerated path (KMEANS_PP_CENTERS and KMEANS_USE_INITIAL_LABELS are outside it)")
    from vision.devmat import to_host_readonly
    data = to_host_readonly(data)
    if not isinstance(data, np.ndarray) or data.ndim != 2 or data.dtype not in (np.uint8, np.float32) or 0 in data.shape:
        raise error("kmeans: (N, d) uint8 or float32 samples only; anything else is outside the accelerated path")
    n, d = data.shape
    if d > 4:
        raise error("kmeans: more than 4 dimensions is outside the accelerated path")
    if n > 1 << 24:
        raise error("kmeans: more than 2^24 samples is outside the accelerated path")
    if data.dtype == np.float32:
        if not (np.isfinite(data).all() and (data >= 0).all() and (data <= 255).all() and (data == np.floor(data)).all()):
            raise error("kmeans: float32 samples that are not integers in 0..255 are outside the accelerated path")
        data = data.astype(np.uint8)
    K, attempts = int(K), int(attempts)
    if K < 1 or K > n:
        raise error("kmeans: K must be in 1..N")
    if K > 256:
        raise error("kmeans: K above 256 is outside the accelerated path")
    if attempts < 1:
        raise error("kmeans: attempts must be at least 1")
    kind, max_count, eps = int(criteria[0]), int(criteria[1]), float(criteria[2])
    max_count = min(max(max_count, 2), 100) if kind & TERM_CRITERIA_COUNT else 100
    eps = max(eps, 0.0) if kind & TERM_CRITERIA_EPS else _FLT_EPSILON
    shape = _kmeans_image_shape(n)
    if shape is None:
        raise error("kmeans: N is not h x w with both sides at most 4096: outside the accelerated path")
    image = np.ascontiguousarray(data).reshape(shape + (d,))
    compactness, labels, found = _gather("kmeans", _color.kmeans, image, K, max_count, eps, seed=0, attempts=attempts)
    labels = np.ascontiguousarray(to_host_readonly(labels)).reshape(n, 1).copy()
    return compactness, _into(bestLabels, labels), _into(centers, found)


# ---- colour-histogram tracking (libvp vp_hist.hip): calcHist, calcBackProject, meanShift, CamShift, DESIGN.md section 4.28 ----------------
NORM_INF, NORM_L1, NORM_L2, NORM_MINMAX = 1, 2, 4, 32


def _one_image(name, images):
    if isinstance(images, (np.ndarray,)) or not isinstance(images, (list, tuple)) or len(images) != 1:
        raise error(f"{name}: a list of exactly one image is on the accelerated path (DESIGN.md section 7)")
    return _source(name, images[0], "only uint8 images are on the accelerated path")


def _vp_call(name, call, *args, **kwargs):
    """what the mirror refuses, and what libvp's entries refuse behind it, is a cv2.error"""
    try:
        return _gather(name, call, *args, **kwargs)
    except _vp.VpError as e:
        raise error(f"{name}: {e}") from e


def calcHist(images, channels, mask, histSize, ranges, hist=None, accumulate=False):
    """cv2.calcHist in cv2's positional order: one uint8 image of 1..4 channels in the list, 1..3 dimensions of 1..256 uniform bins,
    ranges = [low0, high0, ...] with exclusive upper ends; float32 counts, exact.  accumulate, several images, non-uniform ranges and
    non-uint8 images are refused.  A DeviceMat is counted where it is (vision.utils.color.color_histogram)."""
    if accumulate:
        raise error("calcHist: accumulate is not on the accelerated path")
    image = _one_image("calcHist", images)
    return _into(hist, _vp_call("calcHist", _color.color_histogram, image, channels, histSize, ranges, mask))


def calcBackProject(images, channels, hist, ranges, scale, dst=None):
    """cv2.calcBackProject in cv2's positional order: one uint8 image in the list and a dense float32 histogram of 1..3 dimensions;
    uint8 (h, w).  A DeviceMat image gives a DeviceMat that stays in HBM (vision.utils.color.back_project)."""
    image = _one_image("calcBackProject", images)
    return _into(dst, _vp_call("calcBackProject", _color.back_project, image, channels, hist, ranges, scale))


def _shift_criteria(name, criteria):
    """(max_iter, eps) as cv2's meanShift reads a TermCriteria: without the COUNT bit 100 iterations, without the EPS bit eps = 1"""
    try:
        kind, max_count, eps = int(criteria[0]), int(criteria[1]), float(criteria[2])
    except (TypeError, ValueError, IndexError):
        raise error(f"{name}: criteria is (type, maxCount, epsilon)") from None
    return (max(max_count, 1) if kind & TERM_CRITERIA_COUNT else 100), (max(eps, 0.0) if kind & TERM_CRITERIA_EPS else 1.0)


def meanShift(probImage, window, criteria):
    """cv2.meanShift on a uint8 single-channel image: (iterations, window), the loop on the GPU (vision.utils.feature.mean_shift).  A
    window of non-positive size, or with nothing of it inside the image, is refused."""
    max_iter, eps = _shift_criteria("meanShift", criteria)
    return _vp_call("meanShift", _feature.mean_shift, _source("meanShift", probImage, "only uint8 images are on the accelerated path"), window, max_iter, eps)


def CamShift(probImage, window, criteria):
    """cv2.CamShift on a uint8 single-channel image: (((cx, cy), (w, h), angle), window).  The window search and the moments are
    exact integers from the GPU; the box is cv2's double arithmetic on them, through the host's libm."""
    max_iter, eps = _shift_criteria("CamShift", criteria)
    return _vp_call("CamShift", _feature.cam_shift, _source("CamShift", probImage, "only uint8 images are on the accelerated path"), window, max_iter, eps)


OPTFLOW_USE_INITIAL_FLOW = 4
OPTFLOW_LK_GET_MIN_EIGENVALS = 8


def calcOpticalFlowPyrLK(prevImg, nextImg, prevPts, nextPts, status=None, err=None, winSize=(21, 21), maxLevel=3,
                         criteria=(TERM_CRITERIA_COUNT + TERM_CRITERIA_EPS, 30, 0.01), flags=0, minEigThreshold=1e-4):
    """cv2.calcOpticalFlowPyrLK in cv2's positional order on two uint8 single-channel images of one size: (nextPts (N, 1, 2) float32,
    status (N, 1) uint8, err (N, 1) float32), every level and iteration on the GPU (vision.utils.feature.track_points; DESIGN.md
    sections 4.29 and 7).  The images may be numpy arrays, DeviceMats or FlowPyramids.  nextPts is read only with
    OPTFLOW_USE_INITIAL_FLOW.  Without the COUNT bit the criteria mean 30 iterations, without the EPS bit 0.01, as in cv2."""
    try:
        kind, max_count, eps = int(criteria[0]), int(criteria[1]), float(criteria[2])
    except (TypeError, ValueError, IndexError):
        raise error("calcOpticalFlowPyrLK: criteria is (type, maxCount, epsilon)") from None
    try:
        flags = int(flags)
    except (TypeError, ValueError):
        raise error("calcOpticalFlowPyrLK: flags must be an integer") from None
    if flags & ~(OPTFLOW_USE_INITIAL_FLOW | OPTFLOW_LK_GET_MIN_EIGENVALS):
        raise error("calcOpticalFlowPyrLK: unknown flag bits")
    if flags & OPTFLOW_USE_INITIAL_FLOW and nextPts is None:
        raise error("calcOpticalFlowPyrLK: OPTFLOW_USE_INITIAL_FLOW needs nextPts")
    images = [img if isinstance(img, _feature.FlowPyramid) else _source("calcOpticalFlowPyrLK", img, "only uint8 images are on the accelerated path")
              for img in (prevImg, nextImg)]
    found, ok, e = _vp_call("calcOpticalFlowPyrLK", _feature.track_points, images[0], images[1], prevPts, nextPts if flags & OPTFLOW_USE_INITIAL_FLOW else None,
                            winSize, maxLevel, max_count if kind & TERM_CRITERIA_COUNT else 30, eps if kind & TERM_CRITERIA_EPS else 0.01, minEigThreshold,
                            bool(flags & OPTFLOW_LK_GET_MIN_EIGENVALS))
    return (_into(nextPts, found), _into(status, ok.astype(np.uint8).reshape(-1, 1)),
            _into(err, e.reshape(-1, 1)))


LMEDS, RANSAC, RHO = 4, 8, 16


def _motion(name, model, from_, to, method, threshold, maxIters, confidence, allow_plain):
    """(3 x 3 or 2 x 3 float64, (N, 1) uint8 mask), or (None, None) when there is no model"""
    try:
        method = int(method)
    except (TypeError, ValueError):
        raise error(f"{name}: the method must be an integer") from None
    if method in (LMEDS, RHO):
        raise error(f"{name}: LMEDS and RHO are outside the accelerated path (DESIGN.md section 7)")
    if method != RANSAC and not (allow_plain and method == 0):
        raise error(f"{name}: unknown method")
    try:
        src, dst = _feature._motion_pairs(from_, to, _feature._motion_model(model))
        if method == 0:
            M = _feature.refit_motion(src, dst, model)
            return (None, None) if M is None else (M, np.ones((len(src), 1), np.uint8))
    except (ValueError, _vp.VpError) as e:
        raise error(f"{name}: {e}") from None
    try:
        M, inl = _feature.estimate_motion(src, dst, model, threshold, maxIters, confidence)
    except (ValueError, TypeError) as e:
        raise error(f"{name}: {e}") from None
    except _vp.VpError as e:
        raise error(f"{name}: {e}") from e
    return (None, None) if M is None else (M, inl.astype(np.uint8).reshape(-1, 1))


def findHomography(srcPoints, dstPoints, method=0, ransacReprojThreshold=3.0, mask=None, maxIters=2000, confidence=0.995):
    """cv2.findHomography in cv2's positional order for method 0 (the least squares over all pairs, a mask of ones) and RANSAC (the
    search on the GPU, vision.utils.feature.estimate_motion): (H 3 x 3 float64 with H[2, 2] = 1, mask (N, 1) uint8), or (None, None)
    when there is no model.  The contract is the statement of DESIGN.md section 4.30, not cv2's random sequence: the inlier set
    agrees with cv2's where the data decide it; H is the least-squares fit to the inliers without cv2's Levenberg-Marquardt
    polish.  LMEDS and RHO raise."""
    H, inl = _motion("findHomography", "homography", srcPoints, dstPoints, method, ransacReprojThreshold, maxIters, confidence, True)
    return H, (None if inl is None else _into(mask, inl))


def estimateAffine2D(from_, to, inliers=None, method=RANSAC, ransacReprojThreshold=3.0, maxIters=2000, confidence=0.99, refineIters=10):
    """cv2.estimateAffine2D with RANSAC: (M 2 x 3 float64, inliers (N, 1) uint8), or (None, None).  refineIters is accepted and has
    no effect beyond the least-squares fit to the inliers."""
    M, inl = _motion("estimateAffine2D", "affine", from_, to, method, ransacReprojThreshold, maxIters, confidence, False)
    return M, (None if inl is None else _into(inliers, inl))


def estimateAffinePartial2D(from_, to, inliers=None, method=RANSAC, ransacReprojThreshold=3.0, maxIters=2000, confidence=0.99, refineIters=10):
    """cv2.estimateAffinePartial2D with RANSAC: rotation, uniform scale and translation as (M 2 x 3 float64, inliers (N, 1) uint8),
    or (None, None)."""
    M, inl = _motion("estimateAffinePartial2D", "similarity", from_, to, method, ransacReprojThreshold, maxIters, confidence, False)
    return M, (None if inl is None else _into(inliers, inl))


def normalize(src, dst=None, alpha=1.0, beta=0.0, norm_type=NORM_L2, dtype=-1, mask=None):
    """cv2.normalize for NORM_MINMAX on float32 host arrays - what a histogram goes through before calcBackProject: the stretch onto
    [min(alpha, beta), max(alpha, beta)] in double, rounded once (vision.utils.color.normalize_hist; cv2 takes the same steps in
    float32)."""
    if norm_type != NORM_MINMAX:
        raise error("normalize: only NORM_MINMAX is on the accelerated path")
    if mask is not None or dtype not in (-1, CV_32F):
        raise error("normalize: mask= and a dtype other than CV_32F are not on the accelerated path")
    if not isinstance(src, np.ndarray) or src.dtype != np.float32:
        raise error("normalize: only float32 host arrays are on the accelerated path")
    lo, hi = min(float(alpha), float(beta)), max(float(alpha), float(beta))
    return _into(dst, _gather("normalize", _color.normalize_hist, src, hi, lo))


def adaptiveThreshold(src, maxValue, adaptiveMethod, thresholdType, blockSize, C, dst=None):
    """cv2.adaptiveThreshold (utils/color.py:220-292) in cv2's positional order on CV_8UC1 images.  ADAPTIVE_THRESH_MEAN_C: the mean
    path (libvp vp_adaptive_threshold_mean_*, block sizes 3..151); ADAPTIVE_THRESH_GAUSSIAN_C: the exact Gaussian-weighted mean
    (vp_adaptive_threshold_gaussian_*, block sizes 3..511).  A DeviceMat in gives a DeviceMat out."""
    from vision import _vp
    from vision.devmat import DeviceMat, to_host
    from vision.utils.helpers import as_mat
    src = as_mat(src)
    shape = tuple(src.shape) if isinstance(src, (np.ndarray, DeviceMat)) else ()
    if (not isinstance(src, (np.ndarray, DeviceMat)) or src.dtype != np.uint8 or len(shape) not in (2, 3) or (len(shape) == 3 and shape[2] != 1)
            or shape[0] == 0 or shape[1] == 0):
        raise error("adaptiveThreshold: the source must be a non-empty CV_8UC1 image")
    blockSize = int(blockSize)
    if blockSize % 2 != 1 or blockSize <= 1:
        raise error("adaptiveThreshold: blockSize must be odd and greater than 1")
    if maxValue < 0:                               # thresh.cpp: an all-zero result before the method and the type are looked at
        return _into(dst, np.zeros(shape[:2], np.uint8))
    if adaptiveMethod not in (ADAPTIVE_THRESH_MEAN_C, ADAPTIVE_THRESH_GAUSSIAN_C):
        raise error("adaptiveThreshold: unknown or unsupported adaptive threshold method")
    if thresholdType not in (THRESH_BINARY, THRESH_BINARY_INV):
        raise error("adaptiveThreshold: unknown or unsupported threshold type")
    if adaptiveMethod == ADAPTIVE_THRESH_GAUSSIAN_C:
        return _into(dst, _color._adaptive_gaussian(src, blockSize, float(C), int(thresholdType), float(maxValue)))
    if isinstance(src, DeviceMat):                 # the image stays in HBM (libvp vp_adaptive_threshold_mean_dev)
        return _into(dst, _color._adaptive_mean(src, blockSize, float(C), int(thresholdType), float(maxValue)))
    img = np.ascontiguousarray(np.asarray(to_host(src)).reshape(shape[:2]))
    out = np.empty_like(img)
    ctx = _vp.default_context()
    _vp.check(_vp.lib().vp_adaptive_threshold_mean_u8(ctx.handle, _vp.ptr(img), img.shape[1], img.shape[0], float(maxValue), int(thresholdType),
                                                      blockSize, float(C), _vp.ptr(out)), ctx.handle)
    return _into(dst, out)


def threshold(src, thresh, maxval, type, dst=None):
    """cv2.threshold on uint8 images in cv2's positional order -> (retval, dst): THRESH_BINARY, BINARY_INV, TRUNC, TOZERO and
    TOZERO_INV on any channel count (libvp vp_threshold_u8 / _dev; retval is thresh), each optionally with THRESH_OTSU on a single
    channel (vp_otsu_threshold_u8 / _dev; retval is the threshold Otsu's method chose).  A DeviceMat in gives a DeviceMat out."""
    from vision.devmat import DeviceMat
    from vision.utils.helpers import as_mat
    src = as_mat(src)
    try:
        kind = int(type)
    except (TypeError, ValueError):
        raise error("threshold: the threshold type must be an integer") from None
    if kind & THRESH_TRIANGLE:
        raise error("threshold: THRESH_TRIANGLE is outside the accelerated path")
    if (kind & ~(THRESH_MASK | THRESH_OTSU)) or (kind & THRESH_MASK) > THRESH_TOZERO_INV:
        raise error("threshold: unknown threshold type")
    shape = tuple(src.shape) if isinstance(src, (np.ndarray, DeviceMat)) else ()
    if not isinstance(src, (np.ndarray, DeviceMat)) or src.dtype != np.uint8 or len(shape) not in (2, 3) or 0 in shape:
        raise error("threshold: expected a non-empty uint8 image")
    thresh, maxval = float(thresh), float(maxval)
    if thresh != thresh or maxval != maxval:
        raise error("threshold: thresh and maxval must be numbers")
    if kind & THRESH_OTSU:
        if len(shape) == 3 and shape[2] != 1:
            raise error("threshold: THRESH_OTSU takes a CV_8UC1 image")
        t, out = _color._otsu(src, maxval, kind & THRESH_MASK)
        return t, _into(dst, out)
    return thresh, _into(dst, _color._threshold(src, thresh, maxval, kind & THRESH_MASK))


FILLED = -1


def drawContours(image, contours, contourIdx, color, thickness=1):
    """cv2.drawContours: every contour (contourIdx < 0) or the one named; a negative thickness (FILLED) fills each contour by the
    even-odd scanline of vision.utils.draw and outlines it."""
    sel = contours if contourIdx < 0 else [contours[contourIdx]]
    _draw.draw_contours(image, [np.asarray(c) for c in sel], color, thickness)
    return image


def fillPoly(img, pts, color):
    """cv2.fillPoly(img, pts, color) for a list of integer polygons.  Statement of this stand-in (tests/fill_restate.py fill_poly_restate):
    every polygon is filled on its own by the even-odd scanline and outlined, and the image is the union - not one scanline over the
    edges of all polygons together, which cv2 runs: where two polygons of one call overlap, cv2 leaves the overlap unpainted and this
    paints it.  For polygons that do not overlap (and for a single one) the two readings coincide."""
    _draw.draw_contours(img, [np.asarray(p) for p in pts], color, FILLED)
    return img


def fillConvexPoly(img, points, color):
    """cv2.fillConvexPoly: one polygon through the same fill (which does not need it to be convex)."""
    _draw.draw_contours(img, [np.asarray(points)], color, FILLED)
    return img


def boundingRect(array):
    """cv2.boundingRect of integer points: (xmin, ymin, xmax - xmin + 1, ymax - ymin + 1); (0, 0, 0, 0) without points."""
    p = np.asarray(array)
    if not np.issubdtype(p.dtype, np.integer) or (p.size and p.shape[-1] != 2):
        raise error("boundingRect: integer points only on this path")
    p = p.reshape(-1, 2)
    if len(p) == 0:
        return (0, 0, 0, 0)
    x0, y0 = (int(v) for v in p.min(axis=0))
    x1, y1 = (int(v) for v in p.max(axis=0))
    return (x0, y0, x1 - x0 + 1, y1 - y0 + 1)


def convexHull(points, hull=None, clockwise=False, returnPoints=True):
    """cv2.convexHull with returnPoints=True: the hull vertices as an (k, 1, 2) array of the input's dtype.  The vertex SET is cv2's
    (collinear points dropped); the start vertex and the orientation are those of the monotone chain (counter-clockwise from the
    smallest point), not pinned to cv2's, and `clockwise` is not honoured - contourArea of the result, which is all fill_ratio
    (vision_common.py:286) takes, does not depend on either."""
    if not returnPoints:
        raise error("convexHull: returnPoints=False is outside this path")
    p = np.asarray(points)
    out = _convex_hull(p).reshape(-1, 1, 2)
    return out.astype(p.dtype if p.dtype.kind in "iuf" else np.float64)


# ---- keypoints, FAST, brute-force Hamming matching (vision.utils.feature) ---------------------------------
NORM_HAMMING = 6
FAST_FEATURE_DETECTOR_TYPE_9_16 = 2


class KeyPoint:
    """cv2.KeyPoint: pt (x, y), size, angle (-1: none), response, octave, class_id."""
    __slots__ = ("pt", "size", "angle", "response", "octave", "class_id")

    def __init__(self, x=0.0, y=0.0, size=0.0, angle=-1.0, response=0.0, octave=0, class_id=-1):
        self.pt, self.size, self.angle, self.response, self.octave, self.class_id = (float(x), float(y)), float(size), float(angle), float(response), int(octave), int(class_id)

    def __repr__(self):
        return f"KeyPoint(pt={self.pt}, size={self.size}, angle={self.angle}, response={self.response})"


class DMatch:
    """cv2.DMatch: queryIdx, trainIdx, imgIdx, distance."""
    __slots__ = ("queryIdx", "trainIdx", "imgIdx", "distance")

    def __init__(self, queryIdx=-1, trainIdx=-1, imgIdx=-1, distance=float("inf")):
        self.queryIdx, self.trainIdx, self.imgIdx, self.distance = int(queryIdx), int(trainIdx), int(imgIdx), float(distance)

    def __repr__(self):
        return f"DMatch(queryIdx={self.queryIdx}, trainIdx={self.trainIdx}, distance={self.distance})"


KEYPOINT_SIZE = 7.0      # the diameter of the FAST ring, as cv2 reports it


def keypoints_of(pts, scores):
    """the KeyPoint list of fast_corners' arrays: size 7, angle -1, response the score"""
    return [KeyPoint(float(p[0]), float(p[1]), KEYPOINT_SIZE, -1.0, float(s), 0, -1) for p, s in zip(pts, scores)]


class FastFeatureDetector:
    """cv2.FastFeatureDetector for TYPE_9_16 (vision.utils.feature.fast_corners)."""

    def __init__(self, threshold, nonmaxSuppression, type):
        if type != FAST_FEATURE_DETECTOR_TYPE_9_16:
            raise error("FastFeatureDetector_create: only TYPE_9_16 is on the accelerated path (DESIGN.md section 7)")
        self.threshold, self.nonmax = threshold, bool(nonmaxSuppression)

    def detect(self, image, mask=None):
        if mask is not None:
            raise error("FastFeatureDetector.detect: a mask is outside the accelerated path (DESIGN.md section 7)")
        pts, scores = _gather("FastFeatureDetector.detect", _feature.fast_corners, image, self.threshold, self.nonmax)
        return keypoints_of(pts, scores)


def FastFeatureDetector_create(threshold=10, nonmaxSuppression=True, type=FAST_FEATURE_DETECTOR_TYPE_9_16):
    return FastFeatureDetector(threshold, nonmaxSuppression, type)


class BFMatcher:
    """cv2.BFMatcher for NORM_HAMMING on uint8 descriptors (vision.utils.feature.match_descriptors): ties between equal distances go
    to the lower train index.  cv2's default NORM_L2 is not served: a float descriptor has no producer here."""

    def __init__(self, normType=NORM_L2, crossCheck=False):
        if normType != NORM_HAMMING:
            raise error("BFMatcher: only NORM_HAMMING is on the accelerated path; pass it explicitly (DESIGN.md section 7)")
        self.crossCheck = bool(crossCheck)

    def knnMatch(self, queryDescriptors, trainDescriptors, k, mask=None, compactResult=False):
        if mask is not None:
            raise error("BFMatcher.knnMatch: a mask is outside the accelerated path")
        if k > 2:
            raise error("BFMatcher.knnMatch: k above 2 is outside the accelerated path (DESIGN.md section 7)")
        idx, dist = _gather("BFMatcher.knnMatch", _feature.match_descriptors, queryDescriptors, trainDescriptors, k, self.crossCheck)
        return [[DMatch(q, int(j), 0, float(d)) for j, d in zip(idx[q], dist[q]) if j >= 0] for q in range(len(idx))]

    def match(self, queryDescriptors, trainDescriptors, mask=None):
        return [m[0] for m in self.knnMatch(queryDescriptors, trainDescriptors, 1, mask) if m]


def BFMatcher_create(normType=NORM_L2, crossCheck=False):
    return BFMatcher(normType, crossCheck)


def install():
    """Registers this facade as `cv2` when no real OpenCV is importable.  Returns the module that `import cv2` yields.  Every public
    name of this module is then cv2's: the shape descriptors `moments` and `HuMoments` (vision_common.py:131-132) among them."""
    try:
        import cv2 as real
        return real
    except ImportError:
        sys.modules["cv2"] = sys.modules[__name__]
        return sys.modules[__name__]
