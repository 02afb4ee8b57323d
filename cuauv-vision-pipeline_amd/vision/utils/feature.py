"""Mirror of the reference utils/feature.py for the hot path.

`connected_components` is the north-star replacement of the cv2.findContours stage
(utils/feature.py:5-40, modules/red_buoy.py:38): cv2.connectedComponentsWithStats(mask, 8, CV_32S)
semantics on the GPU (libvp vp_ccl_u8).  Polygon helpers (`contour_centroid`, `contour_area`,
utils/feature.py:240-265) are float64 scalar arithmetic on a handful of points and stay on the host.
"""
from typing import List, Tuple

import math
import threading

import numpy as np
from collections.abc import Sequence as _SequenceABC

from vision import _vp
from vision.devmat import DeviceMat, to_host_readonly
from vision.utils.helpers import as_mat, device_image, image_source, run_operator


def connected_components(mat: np.ndarray, numbering: int = _vp.CCL_BLOCK2X2, max_labels: int = 4096,
                         want_labels: bool = True):
    """Returns (nlabels, labels int32 (h,w) or None, stats int32 (k,5), centroids float64 (k,2)),
    k = min(nlabels, max_labels); row 0 is the background, like cv2.  A DeviceMat mask is labelled where it is (libvp vp_ccl_dev, or
    vp_ccl_bits_dev on the bit plane range_threshold left with it): the labels are a DeviceMat too, only the statistics come back."""
    mat = as_mat(mat)
    if isinstance(mat, DeviceMat):
        return _connected_components_dev(mat, numbering, max_labels, want_labels)
    mat = to_host_readonly(mat)
    if not isinstance(mat, np.ndarray) or mat.dtype != np.uint8:
        raise TypeError("expected a uint8 mask")
    if mat.ndim == 3 and mat.shape[2] == 1:
        mat = mat[:, :, 0]
    if mat.ndim != 2 or mat.size == 0:
        raise ValueError("expected a non-empty (h, w) mask")
    if mat.strides[1] != 1:
        mat = np.ascontiguousarray(mat)
    h, w = mat.shape
    labels = np.empty((h, w), np.int32) if want_labels else None
    stats = np.empty((max_labels, 5), np.int32)
    cent = np.empty((max_labels, 2), np.float64)
    n = _vp.C.c_int32(0)
    ctx = _vp.default_context()
    _vp.check(_vp.lib().vp_ccl_u8(ctx.handle, _vp.ptr(mat), mat.strides[0], w, h, int(numbering), _vp.ptr(labels), _vp.ptr(stats),
                                  _vp.ptr(cent), int(max_labels), _vp.C.byref(n)), ctx.handle)
    k = min(n.value, max_labels)
    return n.value, labels, stats[:k].copy(), cent[:k].copy()


def _connected_components_dev(mat, numbering, max_labels, want_labels):
    if mat.dtype != np.uint8:
        raise TypeError("expected a uint8 mask")
    if mat.ndim == 3 and mat.shape[2] == 1:
        mat = mat.reshaped(mat.shape[:2])
    if mat.ndim != 2 or mat.size == 0:
        raise ValueError("expected a non-empty (h, w) mask")
    ctx = _vp.default_context()
    mat.refresh_device(ctx)
    h, w = mat.shape
    labels = DeviceMat(ctx, (h, w), np.int32) if want_labels else None
    stats = np.empty((max_labels, 5), np.int32)
    cent = np.empty((max_labels, 2), np.float64)
    n = _vp.C.c_int32(0)
    lp = labels.dev_ptr if want_labels else None
    bits = mat.bit_plane(ctx)
    if bits is not None and mat._dev_ok and mat._ctx is ctx:       # the same test find_contours uses: the plane still describes the mask
        _vp.check(_vp.lib().vp_ccl_bits_dev(ctx.handle, bits.ptr, w, h, int(numbering), lp, _vp.ptr(stats), _vp.ptr(cent), int(max_labels),
                                            _vp.C.byref(n)), ctx.handle)
    else:
        _vp.check(_vp.lib().vp_ccl_dev(ctx.handle, mat.dev_ptr, w, w, h, int(numbering), lp, _vp.ptr(stats), _vp.ptr(cent), int(max_labels),
                                       _vp.C.byref(n)), ctx.handle)
    k = min(n.value, max_labels)
    return n.value, labels, stats[:k].copy(), cent[:k].copy()


def hist_median(counts) -> np.float64:
    """np.median of the uint8 values whose 256 counters are `counts`: the middle value, or the exact half-sum of the two middle ones."""
    counts = [int(c) for c in counts]
    n = sum(counts)
    if n == 0:
        raise ValueError("median of an empty histogram")
    lo_rank, hi_rank = (n - 1) // 2, n // 2              # ranks (from 0) of the two middle values; equal for odd n
    lo = hi = None
    seen = 0
    for v, c in enumerate(counts):
        seen += c
        if lo is None and seen > lo_rank:
            lo = v
        if seen > hi_rank:
            hi = v
            break
    return np.float64((lo + hi) / 2.0)


def hist_mean(counts) -> np.float64:
    """np.mean of the uint8 values whose 256 counters are `counts`: the exact integer sum divided by the count in float64."""
    counts = [int(c) for c in counts]
    n = sum(counts)
    if n == 0:
        raise ValueError("mean of an empty histogram")
    return np.float64(float(sum(v * c for v, c in enumerate(counts))) / float(n))


def device_histogram(mat) -> np.ndarray:
    """256 counters over all bytes of a uint8 DeviceMat (libvp vp_hist_u8_dev): 1 KB comes back, the image stays in HBM."""
    ctx = _vp.default_context()
    src = device_image(ctx, mat, 0)
    hist = np.zeros(256, np.uint32)
    _vp.check(_vp.lib().vp_hist_u8_dev(ctx.handle, src.dev_ptr, src.size, _vp.ptr(hist)), ctx.handle)
    return hist


_sums_tls = threading.local()


def _green_sums(pts):
    """(a00, a10, a01) of an integer contour as Python ints: one native pass (libvp vp_polygon_sums_i32, host code)."""
    p32 = pts if (pts.dtype == np.int32 and pts.flags.c_contiguous) else np.ascontiguousarray(pts, np.int32)
    t = _sums_tls
    try:
        out, fn = t.out, t.fn
    except AttributeError:                             # per thread: the result buffer and the resolved entry point
        out = t.out = (_vp.C.c_int64 * 3)()
        fn = t.fn = _vp.lib().vp_polygon_sums_i32
    if fn(p32.__array_interface__["data"][0], len(p32), out) != 0:
        raise _vp.VpError("vp_polygon_sums_i32: invalid argument")
    return out[0], out[1], out[2]


def _polygon_moments(contour: np.ndarray):
    """cv2.moments on an (N,1,2) int contour (imgproc/src/moments.cpp contourMoments): Green's theorem,
    float64; m00 made non-negative together with the first moments.  The sums run over integers (coordinates below 2^15, so every
    partial sum stays below 2^53): summed in int64 here, they equal the sequential float64 loop of the C++ code bit for bit."""
    pts = np.asarray(contour).reshape(-1, 2)
    n = len(pts)
    if n == 0:
        return 0.0, 0.0, 0.0
    if not np.issubdtype(pts.dtype, np.integer):
        return _polygon_moments_float(pts.astype(np.float64))
    a00, a10, a01 = (float(v) for v in _green_sums(pts))
    if abs(a00) > 1.1920929e-07:
        if a00 > 0:
            db1_2, db1_6 = 0.5, 1.0 / 6
        else:
            db1_2, db1_6 = -0.5, -1.0 / 6
        return a00 * db1_2, a10 * db1_6, a01 * db1_6
    return 0.0, 0.0, 0.0


def _polygon_moments_float(pts):
    n = len(pts)
    a00 = a10 = a01 = 0.0
    xi_1, yi_1 = pts[n - 1]
    for i in range(n):
        xi, yi = pts[i]
        dxy = xi_1 * yi - xi * yi_1
        a00 += dxy
        a10 += dxy * (xi_1 + xi)
        a01 += dxy * (yi_1 + yi)
        xi_1, yi_1 = xi, yi
    if abs(a00) > 1.1920929e-07:
        if a00 > 0:
            db1_2, db1_6 = 0.5, 1.0 / 6
        else:
            db1_2, db1_6 = -0.5, -1.0 / 6
        return a00 * db1_2, a10 * db1_6, a01 * db1_6
    return 0.0, 0.0, 0.0


# cv2.moments' dictionary, in its order: ten spatial, seven central, seven normalised central moments
MOMENT_FIELDS = ("m00", "m10", "m01", "m20", "m11", "m02", "m30", "m21", "m12", "m03", "mu20", "mu11", "mu02", "mu30", "mu21", "mu12", "mu03",
                 "nu20", "nu11", "nu02", "nu30", "nu21", "nu12", "nu03")


def _complete_moments(sums) -> np.ndarray:
    """(..., 10) spatial moments -> (..., 24) float64 rows in MOMENT_FIELDS order (libvp vp_moments_complete: completeMomentState, host
    code).  Integer sums are rounded to float64 once, here."""
    m = np.ascontiguousarray(sums, np.float64)
    out = np.empty(m.shape[:-1] + (24,), np.float64)
    fn = _vp.lib().vp_moments_complete
    m2, o2 = m.reshape(-1, 10), out.reshape(-1, 24)
    for i in range(len(m2)):
        if fn(m2[i].ctypes.data, o2[i].ctypes.data) != 0:
            raise _vp.VpError("vp_moments_complete: invalid argument")
    return out


def image_moment_sums(mat, binary: bool = False) -> Tuple[int, ...]:
    """The ten spatial moments of a uint8 (h, w) image as exact Python ints, m00 m10 m01 m20 m11 m02 m30 m21 m12 m03: sum x^p y^q v with
    v the pixel, or 1 for a non-zero pixel when `binary` (cv2's binaryImage).  One pass on the GPU (libvp vp_moments_u8 / _dev); a
    DeviceMat is read where it is, and a mask that still carries its bit plane is read through that - the test
    _connected_components_dev uses."""
    mat = as_mat(mat)
    ctx = _vp.default_context()
    out = np.zeros(10, np.uint64)
    if isinstance(mat, DeviceMat):
        src = device_image(ctx, mat, 1)
        h, w = src.shape
        bits = src.bit_plane(ctx) if binary else None
        bp = bits.ptr if (bits is not None and src._dev_ok and src._ctx is ctx) else None
        _vp.check(_vp.lib().vp_moments_dev(ctx.handle, src.dev_ptr, w, w, h, int(bool(binary)), bp, _vp.ptr(out)), ctx.handle)
    else:
        mat = to_host_readonly(mat)
        if not isinstance(mat, np.ndarray) or mat.dtype != np.uint8:
            raise TypeError("expected a uint8 single-channel image")
        if mat.ndim == 3 and mat.shape[2] == 1:
            mat = mat[:, :, 0]
        if mat.ndim != 2 or mat.size == 0:
            raise ValueError("expected a non-empty (h, w) image")
        h, w = mat.shape
        if mat.strides[1] != 1 or (h > 1 and mat.strides[0] < w):
            mat = np.ascontiguousarray(mat)
        _vp.check(_vp.lib().vp_moments_u8(ctx.handle, _vp.ptr(mat), mat.strides[0] if h > 1 else w, w, h, int(bool(binary)), _vp.ptr(out)), ctx.handle)
    return tuple(int(v) for v in out)


def image_moments(mat, binary: bool = False) -> np.ndarray:
    """cv2.moments(image, binaryImage=binary) as a float64 (24,) row in MOMENT_FIELDS order: the exact integer sums of
    image_moment_sums, each rounded to float64 once, then completeMomentState.  `moments_dict` makes cv2's dictionary of it."""
    return _complete_moments(np.array(image_moment_sums(mat, binary), np.uint64))


def component_moment_sums(labels, nlabels: int) -> np.ndarray:
    """(nlabels, 10) uint64: the ten spatial moments of every label value 0 .. nlabels - 1 of an int32 label image, each pixel counting
    1 - one pass on the GPU over all components at once (libvp vp_label_moments_i32 / _dev).  Row 0 is the background; a label outside
    the range counts nowhere.  `labels` is numpy or the DeviceMat connected_components returns."""
    labels = as_mat(labels)
    nlabels = int(nlabels)
    if nlabels < 1:
        raise ValueError("nlabels must be at least 1")
    ctx = _vp.default_context()
    out = np.zeros((nlabels, 10), np.uint64)
    if isinstance(labels, DeviceMat):
        if labels.dtype != np.int32 or labels.ndim != 2 or labels.size == 0:
            raise TypeError("expected a non-empty int32 (h, w) label image")
        labels.refresh_device(ctx)
        h, w = labels.shape
        _vp.check(_vp.lib().vp_label_moments_dev(ctx.handle, labels.dev_ptr, 4 * w, w, h, nlabels, _vp.ptr(out)), ctx.handle)
    else:
        labels = to_host_readonly(labels)
        if not isinstance(labels, np.ndarray) or labels.dtype != np.int32 or labels.ndim != 2 or labels.size == 0:
            raise TypeError("expected a non-empty int32 (h, w) label image")
        labels = np.ascontiguousarray(labels)
        h, w = labels.shape
        _vp.check(_vp.lib().vp_label_moments_i32(ctx.handle, _vp.ptr(labels), 4 * w, w, h, nlabels, _vp.ptr(out)), ctx.handle)
    return out


def component_moments(labels, nlabels: int):
    """(float64 (nlabels, 24) array, MOMENT_FIELDS): cv2.moments(labels == k, binaryImage=True) for every k < nlabels at once, row 0 the
    background.  m00 is the component's area and (m10 / m00, m01 / m00) its centroid, as connected_components reports them."""
    return _complete_moments(component_moment_sums(labels, nlabels)), MOMENT_FIELDS


def contour_moments(contour) -> np.ndarray:
    """cv2.moments(contour) with all 24 fields, a float64 row in MOMENT_FIELDS order: contourMoments' float64 loop (libvp
    vp_polygon_moments, host code) for an (N, 2) or (N, 1, 2) contour of int32 (any integer type) or float32 points, then
    completeMomentState."""
    pts = np.asarray(contour)
    if pts.dtype.kind in "iu":
        pts = np.ascontiguousarray(pts.reshape(-1, 2), np.int32)
    elif pts.dtype == np.float32:
        pts = np.ascontiguousarray(pts.reshape(-1, 2))
    else:
        raise TypeError("expected a contour of int32 or float32 points")
    m = np.empty(10, np.float64)
    if _vp.lib().vp_polygon_moments(pts.ctypes.data if len(pts) else None, int(pts.dtype == np.float32), len(pts), m.ctypes.data) != 0:
        raise _vp.VpError("vp_polygon_moments: invalid argument")
    return _complete_moments(m)


def moments_dict(row) -> dict:
    """cv2.moments' dictionary (24 Python floats, cv2's key order) of one row of image_moments / component_moments / contour_moments."""
    row = np.asarray(row, np.float64).reshape(24)
    return dict(zip(MOMENT_FIELDS, row.tolist()))


def _nu(m):
    if isinstance(m, dict):
        return tuple(float(m[k]) for k in MOMENT_FIELDS[17:])
    return tuple(np.asarray(m, np.float64).reshape(24)[17:].tolist())


def hu_moments(m) -> np.ndarray:
    """cv2.HuMoments of a moments dictionary or 24-field row: float64 (7,), cv::HuMoments' operations in its order."""
    nu20, nu11, nu02, nu30, nu21, nu12, nu03 = _nu(m)
    t0 = nu30 + nu12
    t1 = nu21 + nu03
    q0 = t0 * t0
    q1 = t1 * t1
    n4 = 4 * nu11
    s = nu20 + nu02
    d = nu20 - nu02
    hu = [0.0] * 7
    hu[0] = s
    hu[1] = d * d + n4 * nu11
    hu[3] = q0 + q1
    hu[5] = d * (q0 - q1) + n4 * t0 * t1
    t0 *= q0 - 3 * q1
    t1 *= 3 * q0 - q1
    q0 = nu30 - 3 * nu12
    q1 = 3 * nu21 - nu03
    hu[2] = q0 * q0 + q1 * q1
    hu[4] = q0 * t0 + q1 * t1
    hu[6] = q1 * t0 - q0 * t1
    return np.array(hu, np.float64)


def orientation(m) -> float:
    """Angle of the major axis of a blob from its central moments, 0.5 * atan2(2 mu11, mu20 - mu02), in radians."""
    if isinstance(m, dict):
        mu20, mu11, mu02 = float(m["mu20"]), float(m["mu11"]), float(m["mu02"])
    else:
        mu20, mu11, mu02 = np.asarray(m, np.float64).reshape(24)[10:13].tolist()
    return 0.5 * math.atan2(2 * mu11, mu20 - mu02)


def contour_centroid(contour: np.ndarray) -> Tuple[int, int]:
    """utils/feature.py:240-252."""
    m00, m10, m01 = _polygon_moments(contour)
    m00 = max(1e-10, m00)
    return int(m10 / m00), int(m01 / m00)


def contour_area(contour: np.ndarray) -> float:
    """utils/feature.py:255-265 (cv2.contourArea, oriented=False): |shoelace| / 2."""
    if type(contour) is np.ndarray and contour.dtype == np.int32 and contour.size and contour.flags.c_contiguous:   # what find_contours hands out
        return abs(float(_green_sums(contour.reshape(-1, 2))[0]) * 0.5)
    pts = np.asarray(contour).reshape(-1, 2)
    n = len(pts)
    if n == 0:
        return 0.0
    if np.issubdtype(pts.dtype, np.integer):         # integer sums: exact, equal to the sequential float64 loop (see _polygon_moments)
        return abs(float(_green_sums(pts)[0]) * 0.5)
    pts = pts.astype(np.float64)
    a00 = 0.0
    prev = pts[n - 1]
    for i in range(n):
        p = pts[i]
        a00 += prev[0] * p[1] - prev[1] * p[0]
        prev = p
    return abs(a00 * 0.5)


def contour_perimeter(contour: np.ndarray, closed: bool = True) -> float:
    """utils/feature.py:266-278 (cv2.arcLength): host arithmetic on the few points of one contour."""
    from vision import cv2_facade
    return cv2_facade.arcLength(contour, closed)


def contour_approx(contour: np.ndarray, epsilon: float = None, closed: bool = True) -> np.ndarray:
    """utils/feature.py:281-296 (cv2.approxPolyDP; epsilon defaults to a tenth of the perimeter)."""
    from vision import cv2_facade
    if epsilon is None:
        epsilon = 0.1 * contour_perimeter(contour, closed)
    return cv2_facade.approxPolyDP(contour, epsilon, closed)


def min_enclosing_rect(contour: np.ndarray):
    """utils/feature.py:299-310 (cv2.minAreaRect): ((cx, cy), (w, h), angle in degrees), OpenCV >= 4.5.1 angle convention."""
    from vision import cv2_facade
    return cv2_facade.minAreaRect(contour)


def contour_center(contour: np.ndarray) -> Tuple[float, float]:
    """vision_common.py:290-292: (m10 / m00, m01 / m00) of cv2.moments, unclamped and unrounded - a contour without area divides by
    zero, as it does there."""
    m00, m10, m01 = _polygon_moments(contour)
    return (m10 / m00, m01 / m00)


def is_clipping(mat, contour) -> bool:
    """vision_common.py:271-280: whether the contour's bounding rectangle comes within 5 pixels of an edge of the view."""
    from vision import cv2_facade
    cam_height, cam_width = mat.shape[:2]
    distance = 5
    x, y, w, h = cv2_facade.boundingRect(contour)
    return bool(x <= distance or y <= distance or cam_width - w - x <= distance or cam_height - h - y <= distance)


def fill_ratio(mat, contour, threshed):
    """vision_common.py:282-288: the share of the contour's convex-hull area that is set in `threshed` inside the filled contour -
    drawContours(mask, [contour], -1, 255, thickness=-1), bitwise_and(threshed, threshed, mask=mask), sum / 255 / hull area.
    With `threshed` on the device the mask is made, filled and applied there and one number comes back: the non-zero count
    (vp_count_nonzero_u8_dev) when `threshed` is known to hold only 0 / 255 - sum / 255 is that count then - and otherwise the host sum
    of the masked image, as in the reference."""
    from vision import cv2_facade as cv
    from vision.devmat import lazy_enabled
    from vision.utils import draw
    shape = tuple(int(v) for v in mat.shape[:2])
    hull_area = cv.contourArea(cv.convexHull(contour))
    threshed = as_mat(threshed)
    if isinstance(threshed, DeviceMat) and threshed.dtype == np.uint8 and lazy_enabled() and 0 not in shape:
        ctx = _vp.default_context()
        fill_mask = DeviceMat(ctx, shape, binary=True)
        zero = np.zeros(4, np.uint8)
        _vp.check(_vp.lib().vp_fill_rect_dev(ctx.handle, fill_mask.dev_ptr, shape[1], shape[0], 1, 0, 0, shape[1] - 1, shape[0] - 1, zero.ctypes.data), ctx.handle)
        draw.draw_contours(fill_mask, [np.asarray(contour)], 255, -1)
        fill_masked = cv.bitwise_and(threshed, threshed, mask=fill_mask)
        if threshed.binary:
            return np.float64(cv.countNonZero(fill_masked)) / hull_area
        return np.sum(to_host_readonly(fill_masked)) / 255 / hull_area
    fill_mask = np.zeros(shape, dtype=np.uint8)
    cv.drawContours(fill_mask, [contour], -1, 255, thickness=-1)
    fill_masked = cv.bitwise_and(to_host_readonly(threshed), to_host_readonly(threshed), mask=fill_mask)
    return np.sum(to_host_readonly(fill_masked)) / 255 / hull_area


def _outside_path(name):
    def _f(*_a, **_k):
        raise NotImplementedError(f"{name}: outside the accelerated path of this build")
    _f.__name__ = name
    return _f


min_enclosing_ellipse = _outside_path("min_enclosing_ellipse")


def _circle_points(contour, name):
    """(k, 2) contiguous int32 points within the coordinate bound of the geometry routines; integer-valued floats are taken as integers"""
    p = np.asarray(contour)
    if p.size == 0:
        return np.zeros((0, 2), np.int32)
    p = p.reshape(-1, 2)
    if not np.issubdtype(p.dtype, np.integer):
        q = np.rint(p)
        if not np.array_equal(q, p):
            raise ValueError(f"{name}: integer points only (the support set is found with exact integer predicates)")
        p = q
    if p.min() < _vp.GEOM_COORD_MIN or p.max() > _vp.GEOM_COORD_MAX:
        raise ValueError(f"{name}: coordinates within [{_vp.GEOM_COORD_MIN}, {_vp.GEOM_COORD_MAX}] only")
    return np.ascontiguousarray(p, np.int32)


def min_enclosing_circle(contour: np.ndarray):
    """utils/feature.py:315-325 (cv2.minEnclosingCircle): ((cx, cy), radius) of the smallest circle that contains every point, by libvp's
    host routine - exact integer predicates choose the support points, centre and radius are rounded to float32 once.  OpenCV's small
    safety margin on the radius is not added.  A lone contour does not justify a launch; contour_geometry serves whole lists."""
    p = _circle_points(contour, "min_enclosing_circle")
    out = (_vp.C.c_float * 3)()
    _vp.check(_vp.lib().vp_min_enclosing_circle_i32(p.ctypes.data, len(p), out, None))
    return (out[0], out[1]), out[2]


# one record per contour of contour_geometry
GEOMETRY_DTYPE = np.dtype([("perimeter", np.float64), ("perimeter_open", np.float64), ("hull_count", np.int32), ("hull_area", np.float64),
                           ("rect", np.float32, 5), ("circle", np.float32, 3), ("status", np.uint32)])


def _geometry_table(raw):
    out = np.zeros(raw.shape, GEOMETRY_DTYPE)
    for name in ("perimeter", "perimeter_open", "hull_count", "rect", "circle", "status"):
        out[name] = raw[name]
    out["hull_area"] = raw["hull_area2"] * 0.5
    return out


def _geometry_host_row(rec, pts, hull_out=None):
    """One contour through the host routines: what the device pass leaves to the host (status bits) and what lies outside its bound."""
    from vision import cv2_facade
    p = np.ascontiguousarray(np.asarray(pts).reshape(-1, 2), np.int32)
    if len(p) == 0:
        return                                            # no points: zeros
    rec["perimeter"] = cv2_facade.arcLength(p, True)
    rec["perimeter_open"] = cv2_facade.arcLength(p, False)
    hull = np.empty((max(len(p), 1), 2), np.int32)
    n = _vp.C.c_int(0)
    _vp.check(_vp.lib().vp_convex_hull_i32(p.ctypes.data, len(p), hull.ctypes.data, _vp.C.byref(n)))
    h = hull[:n.value].astype(np.int64)
    rec["hull_count"] = n.value
    rec["hull_area"] = abs(int(np.sum(h[:, 0] * np.roll(h[:, 1], -1) - np.roll(h[:, 0], -1) * h[:, 1]))) * 0.5 if n.value else 0.0
    r5 = (_vp.C.c_float * 5)()
    _vp.check(_vp.lib().vp_min_area_rect_i32(p.ctypes.data, len(p), r5))
    rec["rect"] = np.frombuffer(r5, np.float32)
    if len(p) and p.min() >= _vp.GEOM_COORD_MIN and p.max() <= _vp.GEOM_COORD_MAX:
        c3 = (_vp.C.c_float * 3)()
        _vp.check(_vp.lib().vp_min_enclosing_circle_i32(p.ctypes.data, len(p), c3, None))
        rec["circle"] = np.frombuffer(c3, np.float32)
    else:
        rec["circle"] = np.nan if len(p) else 0.0     # outside the bound of the exact predicates: not computed
    if hull_out is not None:
        hull_out[:n.value] = hull[:n.value]


def _geometry_flat(contours):
    """-> (points (P, 2) int32, counts (K,) int32) of a contour list, without per-contour work where the list carries its block"""
    flat, counts = getattr(contours, "_flat", None), getattr(contours, "_counts", None)
    if flat is not None and counts is not None and flat.dtype == np.int32:
        return np.ascontiguousarray(flat.reshape(-1, 2)), np.ascontiguousarray(counts, np.int32)
    arrs = [np.asarray(c).reshape(-1, 2) for c in contours]
    for a in arrs:
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise TypeError("contour_geometry: integer contours only")
    counts = np.array([len(a) for a in arrs], np.int32)
    flat = np.concatenate(arrs).astype(np.int32, copy=False) if arrs else np.zeros((0, 2), np.int32)
    return np.ascontiguousarray(flat.reshape(-1, 2)), counts


def _geometry_batch(arrs):
    """The arrays of a batched contour pass (ChainRunner's dict: info, counts, offsets, points on the host) through the batch entry:
    staged on the device as the chain leaves them there, (n, max_contours) records back."""
    ctx = _vp.default_context()
    L = _vp.lib()
    info, counts, offsets, points = (np.ascontiguousarray(arrs[k], np.int32) for k in ("info", "counts", "offsets", "points"))
    n, mc, mp = info.shape[0], counts.shape[1], points.shape[1]
    cdesc = _vp.make_contour_desc(max_contours=mc, max_points=mp)
    cb = _vp.ContourBuffers()
    held = []
    try:
        for name, a in (("info", info), ("counts", counts), ("offsets", offsets), ("points", points)):
            p = _vp.C.c_void_p()
            _vp.check(L.vp_dev_alloc(ctx.handle, max(a.nbytes, 8), _vp.C.byref(p)), ctx.handle)
            held.append(p)
            _vp.check(L.vp_memcpy_h2d(ctx.handle, p, a.ctypes.data, a.nbytes), ctx.handle)
            setattr(cb, name, p.value)
        raw = np.zeros((n, mc), _vp.CONTOUR_GEOM_DTYPE)
        _vp.check(L.vp_contour_geometry_batch_dev(ctx.handle, _vp.C.byref(cdesc), _vp.C.byref(cb), n, raw.ctypes.data), ctx.handle)
    finally:
        for p in held:
            L.vp_dev_free(ctx.handle, p)
    out = _geometry_table(raw)
    for f, r in zip(*np.nonzero(raw["status"] & (_vp.GEOM_HULL_CAP | _vp.GEOM_PERIMETER))):
        _geometry_host_row(out[f, r], points[f, offsets[f, r]:offsets[f, r] + counts[f, r]])
    return out


def contour_geometry(contours, hulls: bool = False):
    """Perimeter, convex hull, minimum-area rectangle and minimum enclosing circle of every contour in one device pass (libvp
    vp_contour_geometry_i32): a GEOMETRY_DTYPE record per contour, in the input's order - `perimeter` / `perimeter_open` as
    cv2_facade.arcLength, `hull_count` / `hull_area` of vp_convex_hull_i32's hull, `rect` the five floats of vp_min_area_rect_i32
    (bit for bit), `circle` centre and radius as min_enclosing_circle.  contours: what find_contours returns (its point block is
    passed as it is), any sequence of (N, 1, 2) integer arrays, or the array dict of a batched pass (ChainRunner.carrs: records of
    shape (frames, max_contours), rows that hold no traced contour carry status GEOM_SKIPPED).  Rows the device hands back
    unfinished (status bits) are completed by the host routines before returning.  hulls: also the hull vertices, an int32 block
    laid out like the points - the hull of contour k at the offset of its points, `hull_count` of them."""
    if isinstance(contours, dict):
        if hulls:
            raise ValueError("contour_geometry: the batch form returns no hull vertices")
        return _geometry_batch(contours)
    flat, counts = _geometry_flat(contours)
    k = len(counts)
    raw = np.zeros(k, _vp.CONTOUR_GEOM_DTYPE)
    hull = np.zeros_like(flat) if hulls else None
    if flat.size and (flat.min() < _vp.GEOM_COORD_MIN or flat.max() > _vp.GEOM_COORD_MAX):
        out, o = _geometry_table(raw), 0                      # outside the device pass's bound: the host routines, one by one
        for i, c in enumerate(counts.tolist()):
            _geometry_host_row(out[i], flat[o:o + c], None if hull is None else hull[o:o + c])
            o += c
        return (out, hull) if hulls else out
    if k:
        ctx = _vp.default_context()
        _vp.check(_vp.lib().vp_contour_geometry_i32(ctx.handle, flat.ctypes.data, counts.ctypes.data, k, raw.ctypes.data,
                                                    hull.ctypes.data if hulls else None, None), ctx.handle)
    out = _geometry_table(raw)
    return (out, hull) if hulls else out


def min_enclosing_rects(contours):
    """cv2.minAreaRect of every contour: (K, 5) float32 rows centre x, y, width, height, angle - a view of the contour_geometry table,
    so that a filter like modules/bins.py:33-61 (area, aspect ratio) is array arithmetic over a frame's contours."""
    return contour_geometry(contours)["rect"]


def contour_perimeters(contours, closed: bool = True):
    """cv2.arcLength of every contour: float64 (K,)."""
    return contour_geometry(contours)["perimeter" if closed else "perimeter_open"]


def canny(mat: np.ndarray, lower: int, upper: int) -> np.ndarray:
    """utils/feature.py:43-66 (cv2.Canny with the default 3x3 aperture and L1 gradient) on the GPU (libvp vp_canny_u8).  A device image
    gives a device image (vp_canny_u8_dev), so that canny -> find_lines never visits the host; a numpy image gives numpy."""
    mat = as_mat(mat)
    if isinstance(mat, DeviceMat):
        ctx = _vp.default_context()
        src = device_image(ctx, mat, 0)
        h, w = src.shape[:2]
        cn = 1 if src.ndim == 2 else src.shape[2]
        if cn > 4:
            raise ValueError("canny: at most 4 channels")
        out = DeviceMat(ctx, (h, w), binary=True)
        _vp.check(_vp.lib().vp_canny_u8_dev(ctx.handle, src.dev_ptr, w * cn, w, h, cn, float(lower), float(upper), out.dev_ptr), ctx.handle)
        return out
    from vision import cv2_facade
    return cv2_facade.Canny(mat, lower, upper)


def simple_canny(mat: np.ndarray, sigma: float = 0.33, use_mean: bool = False) -> np.ndarray:
    """utils/feature.py:69-101: thresholds (1 -/+ sigma) x median (or mean) of the image, truncated to int and clamped to [0, 255].  For a
    DeviceMat the statistic comes from the device histogram (all bytes, as numpy's over a multi-channel image)."""
    mat = as_mat(mat)
    if isinstance(mat, DeviceMat) and mat.dtype == np.uint8:
        hist = device_histogram(mat)
        mid = hist_mean(hist) if use_mean else hist_median(hist)
    else:
        mid = np.mean(mat) if use_mean else np.median(mat)
    lower = int(max(0, (1.0 - sigma) * mid))
    upper = int(min(255, (1.0 + sigma) * mid))
    return canny(mat, lower, upper)
# Outside the path on purpose: cv2.HoughLinesP (find_line_segments) draws its points in the order of a seeded RNG and removes each
# segment's votes before the next draw, a serial algorithm by definition.  find_corners and find_circles still raise because the tests of
# this build pin that they do; the operators they wrap are here under their own names: cv2.goodFeaturesToTrack as
# good_features_to_track (with corner_min_eigen_val and corner_harris, the response maps it selects from; cv2_facade.goodFeaturesToTrack,
# cornerMinEigenVal, cornerHarris) - OpenCV's float32 SIMD arithmetic cannot be restated bit for bit, so the contract is the exact value
# of what it approximates, rounded once - and cv2.HoughCircles as hough_circles (cv2_facade.HoughCircles).
find_corners = _outside_path("find_corners")
find_circles = _outside_path("find_circles")
find_line_segments = _outside_path("find_line_segments")

_lines_cap = threading.local()
_circles_cap = threading.local()
_corners_cap = threading.local()

_CORNER_BORDERS = (_vp.BORDER_REFLECT_101, _vp.BORDER_REPLICATE, _vp.BORDER_REFLECT, _vp.BORDER_CONSTANT)
CORNER_MAX_BLOCK = 31


def _corner_block(block_size, ksize=3):
    block_size, ksize = int(block_size), int(ksize)
    if not 1 <= block_size <= CORNER_MAX_BLOCK:
        raise ValueError("blockSize must be in 1..31")
    if ksize != 3:
        raise ValueError("only the 3x3 Sobel (ksize 3) is restated: ksize 5, 7 and -1 (Scharr) are outside the accelerated path")
    return block_size


def _corner_response(name, mat, block_size, ksize, harris, k, border):
    mat, _ = image_source(mat, single=f"{name} takes a single-channel image", max_side=65535)
    block_size = _corner_block(block_size, ksize)
    k, border = float(k), int(border) & ~_vp.BORDER_ISOLATED
    if not math.isfinite(k):
        raise ValueError("k must be finite")
    if border not in _CORNER_BORDERS:
        raise ValueError("the border must be BORDER_REFLECT_101, BORDER_REPLICATE, BORDER_REFLECT or BORDER_CONSTANT")
    h, w = mat.shape
    lib = _vp.lib()
    return run_operator(mat, (h, w), np.float32,
                        lambda ctx, s, d: lib.vp_corner_response_u8(ctx.handle, s, w, w, h, block_size, 3, harris, k, border, d),
                        lambda ctx, s, d: lib.vp_corner_response_dev(ctx.handle, s, w, w, h, block_size, 3, harris, k, border, d))


def corner_min_eigen_val(mat, block_size: int = 3, ksize: int = 3, border: int = _vp.BORDER_REFLECT_101):
    """cv2.cornerMinEigenVal of a uint8 single-channel image as this library defines it: the smaller eigenvalue
    of the block_size x block_size structure tensor of the 3x3 Sobel derivatives - exact integer sums, the eigenvalue in float64 in a
    fixed order, rounded to float32 once - where cv2 runs float32 code that lands near it.  float32 (h, w); numpy in gives numpy out, a
    DeviceMat gives a DeviceMat that stays in HBM (libvp vp_corner_response_*).  Exactly 0 on flat regions and straight edges."""
    return _corner_response("corner_min_eigen_val", mat, block_size, ksize, 0, 0.0, border)


def corner_harris(mat, block_size: int, ksize: int = 3, k: float = 0.04, border: int = _vp.BORDER_REFLECT_101):
    """cv2.cornerHarris under the contract of corner_min_eigen_val: det(M) - k trace(M)^2 of the same structure tensor."""
    return _corner_response("corner_harris", mat, block_size, ksize, 1, k, border)


def good_features_to_track(mat, max_corners: int, quality_thresh: float = 0.01, min_distance: float = 10, mask=None, block_size: int = 3,
                           use_harris: bool = False, k: float = 0.04):
    """cv2.goodFeaturesToTrack(mat, max_corners, quality_thresh, min_distance, mask=mask, blockSize=block_size,
    useHarrisDetector=use_harris, k=k) on the response map of corner_min_eigen_val / corner_harris (utils/feature.py `find_corners`):
    float32 (N, 1, 2) of (x, y), strongest first, or None when there is no corner.  Response, maximum, threshold with the 3 x 3 test and
    the ordering run on the GPU (libvp vp_good_features_*); a device image and a device mask are read where they are (a mask that still
    carries its bit plane through that), and the corners always come back as numpy.  max_corners <= 0 keeps all."""
    mat, _ = image_source(mat, single="good_features_to_track takes a single-channel image", max_side=65535)
    block_size = _corner_block(block_size)
    max_corners, quality, min_distance, k = int(max_corners), float(quality_thresh), float(min_distance), float(k)
    if not (quality > 0 and math.isfinite(quality)):
        raise ValueError("qualityLevel must be positive and finite")
    if not min_distance >= 0:
        raise ValueError("minDistance must be at least 0")
    if not math.isfinite(k):
        raise ValueError("k must be finite")
    h, w = mat.shape
    if mask is not None:
        mask, _ = image_source(mask, single="the mask must be a single-channel image",
                               said=("the mask must be uint8", "the mask must be a non-empty (h, w) image", None))
        if tuple(mask.shape) != (h, w):
            raise ValueError("the mask must have the size of the image")
    ctx = _vp.default_context()
    lib = _vp.lib()
    on_device = isinstance(mat, DeviceMat)
    mp, bp = None, None
    if on_device:
        mat.refresh_device(ctx)
        if mask is not None:
            mask = device_image(ctx, mask, 1)
            bits = mask.bit_plane(ctx)
            bp = bits.ptr if (bits is not None and mask._dev_ok and mask._ctx is ctx) else None
            mp = mask.dev_ptr
    else:
        mat = np.ascontiguousarray(mat)
        if mask is not None:
            mask = np.ascontiguousarray(to_host_readonly(mask))
            mp = mask.ctypes.data
    head = (max_corners, quality, min_distance, mp, w, w if mask is not None else 0, h if mask is not None else 0)
    tail = (block_size, int(bool(use_harris)), k)
    cap = getattr(_corners_cap, "n", 1024)
    if max_corners > 0:
        cap = max_corners
    while True:
        out = np.empty((max(cap, 1), 1, 2), np.float32)
        n = _vp.C.c_int(0)
        if on_device:
            rc = lib.vp_good_features_dev(ctx.handle, mat.dev_ptr, w, w, h, *head, bp, *tail, _vp.ptr(out), cap, _vp.C.byref(n))
        else:
            rc = lib.vp_good_features_u8(ctx.handle, mat.ctypes.data, w, w, h, *head, *tail, _vp.ptr(out), cap, _vp.C.byref(n))
        _vp.check(rc, ctx.handle)
        if n.value <= cap:
            break
        cap = _corners_cap.n = n.value                 # the true count came back: once more with room for all of them
    return out[:n.value].copy() if n.value else None


# ---- distances (libvp vp_dist.hip) ---------------------------------------------------------------------------
DIST_L1, DIST_L2, DIST_C = _vp.DIST_L1, _vp.DIST_L2, _vp.DIST_C
DIST_MAX_SIDE = 4096
_FLOAT_OR_BYTE = (np.dtype(np.uint8), np.dtype(np.float32))


def _valid_bit_plane(mat, ctx):
    """the device pointer of the bit plane a known 0 / 255 mask still carries on ctx, or None"""
    if not mat.binary:
        return None
    bits = mat.bit_plane(ctx)
    return bits.ptr if (bits is not None and mat._dev_ok and mat._ctx is ctx) else None


def _dist_side(mat):
    if max(mat.shape) > DIST_MAX_SIDE:
        raise ValueError("sides above 4096 are outside the accelerated path")


def distance_transform(mat, metric: int = DIST_L2, dst_type=np.float32):
    """cv2.distanceTransform of a uint8 single-channel image: the distance of every pixel to the nearest zero
    pixel.  DIST_L2 is cv2's DIST_MASK_PRECISE value, the correctly rounded float32 root of the exact integer dx^2 + dy^2; DIST_L1 is
    |dx| + |dy| and DIST_C max(|dx|, |dy|), exact integers.  float32 (h, w), or uint8 min(d, 255) for DIST_L1 with dst_type uint8.
    An image without a zero pixel gives +inf (255) everywhere, the distance to the empty set.  Sides up to 4096.  numpy in gives numpy
    out, a DeviceMat gives a DeviceMat that stays in HBM (libvp vp_distance_transform_*); a mask that still carries its bit plane is
    read through that, at an eighth of a byte per pixel."""
    mat, _ = image_source(mat, single="distance_transform takes a single-channel image")
    _dist_side(mat)
    metric, dst_type = int(metric), np.dtype(dst_type)
    if metric not in (DIST_L1, DIST_L2, DIST_C):
        raise ValueError("the metric must be DIST_L1, DIST_L2 or DIST_C")
    if dst_type not in _FLOAT_OR_BYTE:
        raise ValueError("the result must be CV_8U or CV_32F")
    if dst_type == np.uint8 and metric != DIST_L1:
        raise ValueError("a CV_8U result only with DIST_L1")
    depth = _vp.DEPTH_8U if dst_type == np.uint8 else _vp.DEPTH_32F
    h, w = mat.shape
    lib = _vp.lib()

    def on_device(ctx, s, d):
        return lib.vp_distance_transform_dev(ctx.handle, s, w, w, h, _valid_bit_plane(mat, ctx), metric, depth, d, w * dst_type.itemsize)

    return run_operator(mat, (h, w), dst_type, lambda ctx, s, d: lib.vp_distance_transform_u8(ctx.handle, s, w, h, metric, depth, d), on_device)


class _MinMaxLoc(_vp.C.Structure):
    _fields_ = [("min_val", _vp.C.c_double), ("max_val", _vp.C.c_double), ("min_x", _vp.C.c_int), ("min_y", _vp.C.c_int), ("max_x", _vp.C.c_int),
                ("max_y", _vp.C.c_int)]


def min_max_loc(mat, mask=None):
    """cv2.minMaxLoc of a uint8 or float32 single-channel image: (minVal, maxVal, minLoc, maxLoc), Python floats and (x, y) pairs; among
    equal values the first pixel in raster order, at both ends.  mask (uint8, the image's size): only its non-zero pixels take part.
    float32 NaN pixels take no part; +inf and -inf order as numbers.  When no pixel takes part: (0.0, 0.0, (-1, -1), (-1, -1)).  One
    reduction on the GPU (libvp vp_min_max_loc_*): a device image and a device mask are read where they are (a mask that still
    carries its bit plane through that), and 32 bytes come back."""
    mat, _ = image_source(mat, _FLOAT_OR_BYTE, single="min_max_loc takes a single-channel image")
    _dist_side(mat)
    h, w = mat.shape
    if mask is not None:
        mask, _ = image_source(mask, single="the mask must be a single-channel image",
                               said=("the mask must be uint8", "the mask must be a non-empty (h, w) image", None))
        if tuple(mask.shape) != (h, w):
            raise ValueError("the mask must have the size of the image")
    depth = _vp.DEPTH_8U if mat.dtype == np.uint8 else _vp.DEPTH_32F
    ctx = _vp.default_context()
    lib = _vp.lib()
    out = _MinMaxLoc()
    mw, mh = (w, h) if mask is not None else (0, 0)
    if isinstance(mat, DeviceMat):
        mat.refresh_device(ctx)
        mp = bp = None
        if mask is not None:
            mask = device_image(ctx, mask, 1)
            bp = _valid_bit_plane(mask, ctx)
            mp = mask.dev_ptr
        rc = lib.vp_min_max_loc_dev(ctx.handle, mat.dev_ptr, w * mat.itemsize, w, h, depth, mp, w, mw, mh, bp, _vp.C.addressof(out))
    else:
        mat = np.ascontiguousarray(mat)
        if mask is not None:
            mask = np.ascontiguousarray(to_host_readonly(mask))
        rc = lib.vp_min_max_loc_u8(ctx.handle, mat.ctypes.data, w * mat.itemsize, w, h, depth, None if mask is None else mask.ctypes.data, w, mw, mh,
                                   _vp.C.addressof(out))
    _vp.check(rc, ctx.handle)
    return out.min_val, out.max_val, (out.min_x, out.min_y), (out.max_x, out.max_y)


def largest_inscribed_circle(mask):
    """((x, y), radius) of the largest circle inside the non-zero region of a uint8 mask: distance_transform (DIST_L2) followed by
    min_max_loc, the first deepest pixel in raster order.  The radius is the distance from that pixel's centre to the centre of the
    nearest zero pixel, so a disc drawn with it just touches that pixel.  A DeviceMat mask never visits the host in between: the float32
    map stays in HBM and 32 bytes come back.  A mask without a zero pixel is refused (ValueError): the radius would be infinite."""
    _, radius, _, centre = min_max_loc(distance_transform(mask, DIST_L2))
    if math.isinf(radius):
        raise ValueError("the mask has no zero pixel: the largest inscribed circle is unbounded")
    return centre, radius


# ---- template matching (libvp vp_match.hip) --------------------------------------------------------------------
TM_SQDIFF, TM_SQDIFF_NORMED, TM_CCORR, TM_CCORR_NORMED, TM_CCOEFF, TM_CCOEFF_NORMED = range(6)
MATCH_MAX_SIDE, MATCH_MAX_ELEMS = 4096, 65536


class DeviceCrop:
    """The window (x, y, w, h) of a device image, as a template that match_template reads where it lies (no copy is made): a patch of
    an earlier frame that is still in HBM."""
    __slots__ = ("mat", "x", "y", "w", "h")

    def __init__(self, mat, x: int, y: int, w: int, h: int):
        if not isinstance(mat, DeviceMat) or mat.dtype != np.uint8 or mat.ndim not in (2, 3):
            raise TypeError("a DeviceCrop is a window of a uint8 DeviceMat image")
        x, y, w, h = int(x), int(y), int(w), int(h)
        if w < 1 or h < 1 or x < 0 or y < 0 or x + w > mat.shape[1] or y + h > mat.shape[0]:
            raise ValueError("the window must lie inside the image and hold a pixel")
        self.mat, self.x, self.y, self.w, self.h = mat, x, y, w, h

    @property
    def shape(self):
        return (self.h, self.w) + tuple(self.mat.shape[2:])


def _match_template_args(mat, templ, method):
    """the checked image, template and their sizes; everything match_template refuses is refused here, before a device is needed"""
    mat, cn = image_source(mat, max_side=MATCH_MAX_SIDE)
    crop = templ if isinstance(templ, DeviceCrop) else None
    if crop is None:
        templ, tcn = image_source(templ, said=("the template must be uint8", "the template must be a non-empty (h, w) or (h, w, c) image", "at most 4 channels"))
        th, tw = templ.shape[:2]
    else:
        tcn = 1 if crop.mat.ndim == 2 else crop.mat.shape[2]
        th, tw = crop.h, crop.w
    method = int(method)
    if method not in range(6):
        raise ValueError("the method must be one of the six TM_* values")
    if tcn != cn:
        raise ValueError("the image and the template must have the same number of channels")
    h, w = mat.shape[:2]
    if th > h or tw > w:
        raise ValueError("the template is larger than the image")
    if tw * th * cn > MATCH_MAX_ELEMS:
        raise ValueError("templates above 65536 bytes (tw * th * channels) are outside the accelerated path")
    return mat, templ, cn, w, h, tw, th, method


def match_template(mat, templ, method: int = TM_CCOEFF_NORMED):
    """cv2.matchTemplate of a uint8 image and a uint8 template of the same 1..4 channels: the float32 map of
    (h - th + 1, w - tw + 1) scores by one of the six TM_* methods.  The sums under every score are exact integers and the arithmetic
    after them is cv2's in double, rounded to float32 once; cv2 itself correlates by a float32 DFT and approximates these values.
    Image sides up to 4096, templates up to 65536 bytes.  numpy in gives numpy out; a DeviceMat image gives a DeviceMat that stays in
    HBM (libvp vp_match_template_*).  A numpy template is uploaded; a DeviceMat or a DeviceCrop template is read where it lies."""
    mat, templ, cn, w, h, tw, th, method = _match_template_args(mat, templ, method)
    lib = _vp.lib()
    if not isinstance(mat, DeviceMat):
        t = np.ascontiguousarray(to_host_readonly(templ.mat)[templ.y:templ.y + th, templ.x:templ.x + tw] if isinstance(templ, DeviceCrop)
                                 else to_host_readonly(templ))
        return run_operator(mat, (h - th + 1, w - tw + 1), np.float32,
                            lambda ctx, s, d: lib.vp_match_template_u8(ctx.handle, s, w, h, cn, t.ctypes.data, tw, th, method, d), None)

    def on_device(ctx, s, d):
        if isinstance(templ, DeviceCrop):
            templ.mat.refresh_device(ctx)
            tp, ts = templ.mat.dev_ptr + (templ.y * templ.mat.shape[1] + templ.x) * cn, templ.mat.shape[1] * cn
        else:
            held = device_image(ctx, templ, 0)               # (an uploaded template lives until the call is queued)
            tp, ts = held.dev_ptr, tw * cn
        return lib.vp_match_template_dev(ctx.handle, s, w * cn, w, h, cn, tp, ts, tw, th, method, d, (w - tw + 1) * 4)

    return run_operator(mat, (h - th + 1, w - tw + 1), np.float32, None, on_device)


def best_match(mat, templ, method: int = TM_CCOEFF_NORMED):
    """((x, y), score) of the best match of templ in mat: match_template followed by min_max_loc - the minimum for the two SQDIFF
    methods, the maximum otherwise, the first pixel in raster order among equal scores.  (x, y) is the top-left corner of the matched
    window.  With a device image the score map never visits the host: it stays in HBM and 32 bytes come back."""
    lo, hi, lo_at, hi_at = min_max_loc(match_template(mat, templ, method))
    return (lo_at, lo) if int(method) in (TM_SQDIFF, TM_SQDIFF_NORMED) else (hi_at, hi)


# ---- mean shift and CamShift (libvp vp_hist.hip) ----------------------------------------------------------------
MEAN_SHIFT_MAX_SIDE, MEAN_SHIFT_MAX_WINDOWS, MEAN_SHIFT_MAX_ITER = 4096, 4096, 100000
CAM_SHIFT_TOLERANCE = 10


def _clip_window(win, cols, rows):
    """(x, y, w, h) cut to the image, or None when nothing is left"""
    x, y, w, h = win
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, cols), min(y + h, rows)
    return (x0, y0, x1 - x0, y1 - y0) if x1 > x0 and y1 > y0 else None


def _mean_shift_args(prob, windows, max_iter, eps):
    """the checked image and windows; everything vp_mean_shift_dev refuses is refused here, before a device is needed"""
    prob, _ = image_source(prob, single="mean shift takes a single-channel image", max_side=MEAN_SHIFT_MAX_SIDE)
    rows, cols = prob.shape
    try:
        wins = np.array([[int(v) for v in win] for win in windows], np.int64).reshape(-1, 4)
    except (TypeError, ValueError):
        raise ValueError("a window is four integers (x, y, w, h)") from None
    if not 1 <= len(wins) <= MEAN_SHIFT_MAX_WINDOWS:
        raise ValueError("1 to 4096 windows")
    if np.abs(wins).max() >= 2 ** 31:
        raise ValueError("a window is four 32-bit integers")
    for win in wins:
        if win[2] <= 0 or win[3] <= 0:
            raise ValueError("a window has a non-positive size")
        if _clip_window(tuple(int(v) for v in win), cols, rows) is None:
            raise ValueError("a window is empty inside the image")
    max_iter, eps = int(max_iter), float(eps)
    if max_iter > MEAN_SHIFT_MAX_ITER:
        raise ValueError("more than 100000 iterations are outside the accelerated path")
    return prob, np.ascontiguousarray(wins.astype(np.int32)), max_iter, (eps if eps == eps else 0.0)


def mean_shift_many(prob, windows, max_iter: int = 10, eps: float = 1.0):
    """cv2.meanShift of a batch of windows (x, y, w, h) over one uint8 single-channel image, in one launch with one block per window
    and the whole loop on the GPU (libvp vp_mean_shift_dev): a list of (iterations, window).  A DeviceMat is
    read where it is; only five integers per window come back.  max_iter below 1 counts as 1; eps below 0 as 0."""
    prob, wins, max_iter, eps = _mean_shift_args(prob, windows, max_iter, eps)
    rows, cols = prob.shape
    ctx = _vp.default_context()
    src = device_image(ctx, prob, 1)
    out = np.empty((len(wins), 5), np.int32)
    _vp.check(_vp.lib().vp_mean_shift_dev(ctx.handle, src.dev_ptr, cols, cols, rows, wins.ctypes.data, len(wins), max_iter, eps, None, out.ctypes.data), ctx.handle)
    return [(int(r[4]), (int(r[0]), int(r[1]), int(r[2]), int(r[3]))) for r in out]


def mean_shift(prob, window, max_iter: int = 10, eps: float = 1.0):
    """cv2.meanShift(prob, window, (COUNT | EPS, max_iter, eps)): (iterations, window) - mean_shift_many of one window."""
    return mean_shift_many(prob, [window], max_iter, eps)[0]


def _round_half_even(v: float) -> int:
    return int(np.rint(v))


def cam_shift_box(sums, window, cols: int, rows: int):
    """The finishing arithmetic of cv2.CamShift, in double on the host, from the ten exact raster sums of the grown window
    (x, y, w, h): (((cx, cy), (w, h), angle), window).  atan2, cos, sin and sqrt are the host's libm."""
    m00, m10, m01, m20, m11, m02 = (float(int(s)) for s in sums[:6])
    x, y, w, h = window
    if abs(m00) < 2.220446049250313e-16:
        return ((0.0, 0.0), (0.0, 0.0), 0.0), window
    inv_m00 = 1.0 / m00
    mx, my = m10 * inv_m00, m01 * inv_m00
    mu20, mu11, mu02 = m20 - m10 * mx, m11 - m10 * my, m02 - m01 * my
    xc, yc = _round_half_even(m10 * inv_m00 + x), _round_half_even(m01 * inv_m00 + y)
    a, b, c = mu20 * inv_m00, mu11 * inv_m00, mu02 * inv_m00
    square = math.sqrt(4 * b * b + (a - c) * (a - c))
    theta = math.atan2(2 * b, a - c + square)
    cs, sn = math.cos(theta), math.sin(theta)
    rotate_a = max(0.0, cs * cs * mu20 + 2 * cs * sn * mu11 + sn * sn * mu02)
    rotate_c = max(0.0, sn * sn * mu20 - 2 * cs * sn * mu11 + cs * cs * mu02)
    length, width = math.sqrt(rotate_a * inv_m00) * 4, math.sqrt(rotate_c * inv_m00) * 4
    if length < width:
        length, width = width, length
        cs, sn = sn, cs
        theta = math.pi * 0.5 - theta
    t0 = max(_round_half_even(abs(length * cs)), _round_half_even(abs(width * sn))) + 2
    w = min(t0, (cols - xc) * 2)
    t0 = max(_round_half_even(abs(length * sn)), _round_half_even(abs(width * cs))) + 2
    h = min(t0, (rows - yc) * 2)
    x, y = max(0, xc - int(w / 2)), max(0, yc - int(h / 2))
    w, h = min(cols - x, w), min(rows - y, h)
    angle = np.float32((math.pi * 0.5 + theta) * 180.0 / math.pi)
    while angle < 0:
        angle = np.float32(angle + np.float32(360))
    while angle >= 360:
        angle = np.float32(angle - np.float32(360))
    if angle >= 180:
        angle = np.float32(angle - np.float32(180))
    centre = (float(np.float32(x) + np.float32(w) * np.float32(0.5)), float(np.float32(y) + np.float32(h) * np.float32(0.5)))
    return (centre, (float(np.float32(width)), float(np.float32(length))), float(angle)), (x, y, w, h)


def cam_shift(prob, window, max_iter: int = 10, eps: float = 1.0):
    """cv2.CamShift(prob, window, (COUNT | EPS, max_iter, eps)): (((cx, cy), (w, h), angle), window).  mean_shift, then the exact
    raster sums of the found window grown by 10 pixels on every side (libvp vp_moments_dev on that part of the device image) - the
    integers come from the GPU; the double arithmetic after them (cam_shift_box) runs on the host and goes through its libm."""
    prob = _mean_shift_args(prob, [window], max_iter, eps)[0]
    rows, cols = prob.shape
    ctx = _vp.default_context()
    src = device_image(ctx, prob, 1)
    _, (x, y, w, h) = mean_shift(src, window, max_iter, eps)
    x, y = max(x - CAM_SHIFT_TOLERANCE, 0), max(y - CAM_SHIFT_TOLERANCE, 0)
    w, h = min(w + 2 * CAM_SHIFT_TOLERANCE, cols - x), min(h + 2 * CAM_SHIFT_TOLERANCE, rows - y)
    sums = np.zeros(10, np.uint64)
    _vp.check(_vp.lib().vp_moments_dev(ctx.handle, src.dev_ptr + y * cols + x, cols, w, h, 0, None, sums.ctypes.data), ctx.handle)
    return cam_shift_box(sums, (x, y, w, h), cols, rows)


# ---- sparse optical flow (libvp vp_flow.hip) --------------------------------------------------------------------
OPTFLOW_USE_INITIAL_FLOW, OPTFLOW_LK_GET_MIN_EIGENVALS = 4, 8
FLOW_MAX_SIDE, FLOW_MAX_POINTS, FLOW_MIN_WIN, FLOW_MAX_WIN, FLOW_MAX_LEVEL = 4096, 1 << 20, 3, 63, 15


def _flow_window(win_size):
    try:
        ww, wh = (int(v) for v in win_size)
    except (TypeError, ValueError):
        raise ValueError("the window is two integers (width, height)") from None
    if not (FLOW_MIN_WIN <= ww <= FLOW_MAX_WIN and FLOW_MIN_WIN <= wh <= FLOW_MAX_WIN):
        raise ValueError("a window side must be 3 to 63")
    return ww, wh


def _flow_max_level(max_level):
    max_level = int(max_level)
    if not 0 <= max_level <= FLOW_MAX_LEVEL:
        raise ValueError("maxLevel must be 0 to 15")
    return max_level


def flow_level_count(w: int, h: int, win_size=(21, 21), max_level: int = 3) -> int:
    """How many pyramid levels track_points uses on a w x h image: level l exists while its width is above the window's and its height
    above the window's, up to max_level; 0 when the image itself is not larger than the window."""
    ww, wh = win_size
    n = 0
    while n <= max_level and w > ww and h > wh:
        n, w, h = n + 1, (w + 1) // 2, (h + 1) // 2
    return n


def _flow_source(mat):
    """the checked level 0 of a pyramid - a numpy image, a DeviceMat or a DeviceCrop - and its (h, w); no device is needed"""
    if isinstance(mat, DeviceCrop):
        if mat.mat.ndim != 2:
            raise ValueError("track_points takes single-channel images")
        if max(mat.h, mat.w) > FLOW_MAX_SIDE:
            raise ValueError(f"the source must be at most {FLOW_MAX_SIDE} x {FLOW_MAX_SIDE}")
        return mat, (mat.h, mat.w)
    mat, _ = image_source(mat, single="track_points takes single-channel images", max_side=FLOW_MAX_SIDE)
    return mat, tuple(mat.shape)


class FlowPyramid:
    """The levels of one frame for track_points, kept in HBM: level 0 is the frame (a numpy image is uploaded once, a DeviceMat or a
    DeviceCrop - a window of a wider device image - is read where it lies), level l + 1 is pyr_down of level l.  Only the levels
    that exist for `win_size` up to `max_level` are made.  The pyramid of frame t + 1 serves as `next` in one call and as `prev` in
    the following one: each frame is reduced once."""

    def __init__(self, mat, max_level: int = 3, win_size=(21, 21)):
        ww, wh = _flow_window(win_size)
        max_level = _flow_max_level(max_level)
        mat, (h, w) = _flow_source(mat)
        crop = mat if isinstance(mat, DeviceCrop) else None
        count = flow_level_count(w, h, (ww, wh), max_level)
        if count == 0:
            raise ValueError("the image must be larger than the window")
        ctx = _vp.default_context()
        lib = _vp.lib()
        if crop is not None:
            crop.mat.refresh_device(ctx)
            held, ptr, stride = crop.mat, crop.mat.dev_ptr + crop.y * crop.mat.shape[1] + crop.x, crop.mat.shape[1]
        else:
            held = device_image(ctx, mat, 1)
            ptr, stride = held.dev_ptr, w
        self.ctx, self.shape, self.win_size, self.max_level = ctx, (h, w), (ww, wh), max_level
        self.levels = [(ptr, stride, w, h)]           # (device pointer, bytes between rows, columns, rows)
        self._held = [held]
        for _ in range(count - 1):
            ptr, stride, w, h = self.levels[-1]
            down = DeviceMat(ctx, ((h + 1) // 2, (w + 1) // 2))
            _vp.check(lib.vp_pyr_down_dev(ctx.handle, ptr, stride, w, h, 1, _vp.BORDER_REFLECT_101, down.dev_ptr), ctx.handle)
            self.levels.append((down.dev_ptr, (w + 1) // 2, (w + 1) // 2, (h + 1) // 2))
            self._held.append(down)

    def __len__(self):
        return len(self.levels)


def _flow_points(pts, what):
    try:
        pts = np.asarray(pts, np.float32)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be float32 (x, y) pairs") from None
    if pts.size % 2 or (pts.ndim and pts.shape[-1] != 2 and pts.size):
        raise ValueError(f"{what} must be float32 (x, y) pairs")
    return np.ascontiguousarray(pts.reshape(-1, 2))


def _flow_launch(P, Q, count, pts, guess, win, max_level, max_count, eps, flags, min_eig):
    """one launch over `count` levels of the pyramids P (first image) and Q (second): (positions (n, 2), status (n,) bool, err (n,))"""
    ctx = P.ctx
    n = len(pts)
    ptrs = lambda pyr: ((_vp.C.c_void_p * count)(*[lv[0] for lv in pyr.levels[:count]]), (_vp.C.c_size_t * count)(*[lv[1] for lv in pyr.levels[:count]]))
    (pp, ps), (qp, qs) = ptrs(P), ptrs(Q)
    out = np.empty((n, 4), np.uint32)
    h, w = P.shape
    _vp.check(_vp.lib().vp_lk_flow_dev(ctx.handle, pp, ps, qp, qs, count, w, h, pts.ctypes.data, None if guess is None else guess.ctypes.data, n, win[0], win[1],
                                       max_level, max_count, eps, flags, min_eig, None, out.ctypes.data), ctx.handle)
    return out[:, :2].copy().view(np.float32), out[:, 3] != 0, out[:, 2].copy().view(np.float32)


def track_points(prev, next, pts, next_pts=None, win_size=(21, 21), max_level: int = 3, max_count: int = 30, eps: float = 0.01, min_eig_threshold: float = 1e-4,
                 min_eigenvals: bool = False, back_check=None):
    """cv2.calcOpticalFlowPyrLK: follows the points `pts` of the uint8 single-channel image `prev` into `next` by pyramidal
    Lucas-Kanade (libvp vp_lk_flow_dev, one launch with one wave per point and every level inside it).
    Returns (next_pts (N, 1, 2) float32, status (N,) bool, err (N,) float32) as numpy.  The window sums are exact integers and what
    follows them is cv2's sequence in double in one fixed order: the exact value of what cv2's float32 code approximates.
    prev and next are numpy images, DeviceMats, DeviceCrops or FlowPyramids; a FlowPyramid is used as it is, so that a frame is
    reduced once however many calls it takes part in.  next_pts: starting positions (cv2's OPTFLOW_USE_INITIAL_FLOW).  max_count is
    clamped to 0..100 and eps to 0..10, as cv2 clamps its TermCriteria.  err is the mean absolute difference of the window at the
    final position (0 for a lost point), or with min_eigenvals the minimum eigenvalue at level 0.  back_check=t tracks the results
    back into `prev` (a second launch over the same pyramids) and clears the status of points that return more than t pixels from
    their start, or not at all.  A point with a coordinate that is not finite or beyond +-2^24 is lost and comes back unchanged."""
    win = _flow_window(win_size)
    max_level = _flow_max_level(max_level)
    max_count, eps, min_eig = int(max_count), float(eps), float(min_eig_threshold)
    if not (math.isfinite(eps) and math.isfinite(min_eig)):
        raise ValueError("epsilon and minEigThreshold must be finite")
    if back_check is not None:
        back_check = float(back_check)
        if not back_check >= 0:
            raise ValueError("back_check must be at least 0")
    pts = _flow_points(pts, "the points")
    guess = None
    if next_pts is not None:
        guess = _flow_points(next_pts, "the initial positions")
        if guess.shape != pts.shape:
            raise ValueError("as many initial positions as points")
    if len(pts) > FLOW_MAX_POINTS:
        raise ValueError("more than 1048576 points are outside the accelerated path")
    shapes = [x.shape if isinstance(x, FlowPyramid) else _flow_source(x)[1] for x in (prev, next)]
    if shapes[0] != shapes[1]:
        raise ValueError("the two images must have the same size")
    count = flow_level_count(shapes[0][1], shapes[0][0], win, max_level)
    if count == 0:
        raise ValueError("the image must be larger than the window")
    P = prev if isinstance(prev, FlowPyramid) else FlowPyramid(prev, max_level, win)       # (everything above is refused before a device is needed)
    Q = next if isinstance(next, FlowPyramid) else FlowPyramid(next, max_level, win)
    if min(len(P), len(Q)) < count or P.ctx is not Q.ctx:
        raise ValueError("a FlowPyramid holds fewer levels than this call uses (or lives on another context): make it with this window and maxLevel")
    if len(pts) == 0:
        return np.empty((0, 1, 2), np.float32), np.empty(0, bool), np.empty(0, np.float32)
    flags = (OPTFLOW_USE_INITIAL_FLOW if guess is not None else 0) | (OPTFLOW_LK_GET_MIN_EIGENVALS if min_eigenvals else 0)
    found, status, err = _flow_launch(P, Q, count, pts, guess, win, max_level, max_count, eps, flags, min_eig)
    if back_check is not None:
        back, back_ok, _ = _flow_launch(Q, P, count, np.ascontiguousarray(found), None, win, max_level, max_count, eps, 0, min_eig)
        d = back.astype(np.float64) - pts.astype(np.float64)
        with np.errstate(all="ignore"):
            status = status & back_ok & ~(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] > back_check * back_check)
    return found.reshape(-1, 1, 2), status, err


# ---- robust motion estimation from point pairs (libvp vp_model.hip) ------------------------------------------
MOTION_MODELS = {"similarity": _vp.MODEL_SIMILARITY, "affine": _vp.MODEL_AFFINE, "homography": _vp.MODEL_HOMOGRAPHY}
MOTION_MAX_POINTS, MOTION_MAX_ITERS = 1 << 20, 65536


def _motion_model(model):
    if model not in MOTION_MODELS:
        raise ValueError("the model is 'similarity', 'affine' or 'homography'")
    return MOTION_MODELS[model]


def _motion_pairs(src_pts, dst_pts, model, status=None):
    """the checked (N, 2) float32 pairs of a motion model, lost points left out; no device is needed"""
    src, dst = _flow_points(src_pts, "the source points"), _flow_points(dst_pts, "the destination points")
    if len(src) != len(dst):
        raise ValueError("as many destination points as source points")
    if status is not None:
        keep = np.asarray(status).reshape(-1) != 0
        if len(keep) != len(src):
            raise ValueError("one status per point pair")
        src, dst = np.ascontiguousarray(src[keep]), np.ascontiguousarray(dst[keep])
    if len(src) < model + 2:
        raise ValueError(f"the model needs at least {model + 2} point pairs")
    if len(src) > MOTION_MAX_POINTS:
        raise ValueError("more than 1048576 point pairs are outside the accelerated path")
    return src, dst


def _motion_matrix(model, nine):
    return nine.reshape(3, 3).copy() if model == _vp.MODEL_HOMOGRAPHY else nine.reshape(3, 3)[:2].copy()


def estimate_motion(src_pts, dst_pts, model: str = "similarity", threshold: float = 3.0, max_iters: int = 2000, confidence: float = 0.99, seed: int = 0,
                    status=None):
    """The motion between two point sets by RANSAC on the GPU - what cv2.estimateAffinePartial2D ("similarity"), estimateAffine2D
    ("affine") and findHomography ("homography") make of point pairs (libvp vp_estimate_model_f32).  Returns
    (M, inliers): M is 2 x 3 float64 for the similarity and the affine model and 3 x 3 for the homography, the least-squares fit to
    the inlier set of the best hypothesis; inliers is (N,) bool.  (None, None) when there is no model.  The points are (N, 2) or
    (N, 1, 2), float32 or convertible; status= takes track_points' status and leaves lost points out (inliers then has one entry per
    kept point).  The result is a function of the arguments alone, bit for bit (tests/model_restate.py): hypothesis j draws its
    sample from (seed, j), ties go to the lowest j, and the search ends by cv2's rule for `confidence`, checked every 256 hypotheses."""
    kind = _motion_model(model)
    threshold, max_iters, confidence, seed = float(threshold), int(max_iters), float(confidence), int(seed)
    if not (math.isfinite(threshold) and threshold > 0):
        raise ValueError("the threshold must be finite and above 0")
    if not 1 <= max_iters <= MOTION_MAX_ITERS:
        raise ValueError("max_iters must be 1 to 65536")
    if not 0 < confidence < 1:
        raise ValueError("the confidence must be above 0 and below 1")
    if not 0 <= seed < 1 << 32:
        raise ValueError("the seed is an unsigned 32-bit integer")
    src, dst = _motion_pairs(src_pts, dst_pts, kind, status)
    ctx = _vp.default_context()
    nine, mask = np.empty(9, np.float64), np.empty(len(src), np.uint8)
    count, taken = _vp.C.c_int(), _vp.C.c_int()
    _vp.check(_vp.lib().vp_estimate_model_f32(ctx.handle, src.ctypes.data, dst.ctypes.data, len(src), kind, threshold, max_iters, confidence, seed, nine.ctypes.data,
                                              mask.ctypes.data, _vp.C.addressof(count), _vp.C.addressof(taken)), ctx.handle)
    if count.value == 0:
        return None, None
    return _motion_matrix(kind, nine), mask != 0


def refit_motion(src_pts, dst_pts, model: str = "similarity", mask=None):
    """The plain least-squares model over the pairs whose mask entry is not 0 (all without a mask), in double on the host in index
    order (libvp vp_model_refit): 2 x 3 or 3 x 3 float64, or None when the points do not determine the model."""
    kind = _motion_model(model)
    src, dst = _motion_pairs(src_pts, dst_pts, kind)
    if mask is not None:
        mask = np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, np.uint8)
        if len(mask) != len(src):
            raise ValueError("one mask entry per point pair")
    nine = np.empty(9, np.float64)
    rc = _vp.lib().vp_model_refit(src.ctypes.data, dst.ctypes.data, len(src), None if mask is None else mask.ctypes.data, kind, nine.ctypes.data)
    if rc < 0:
        _vp.check(rc)
    return _motion_matrix(kind, nine) if rc == 1 else None


# ---- FAST corners, steered binary descriptors, Hamming matching (libvp vp_features.hip) ----------------------
FEATURE_MAX_SIDE, FEATURE_MAX_PIXELS, FEATURE_MAX_POINTS = 65535, 1 << 28, 1 << 20
FAST_MIN_SIDE, DESCRIBE_MIN_SIDE, DESCRIPTOR_BYTES = 7, 31, 32
HAMMING_MAX_BYTES, HAMMING_MAX_ROWS = 128, 1 << 20
_fast_cap = threading.local()


def _feature_image(mat, name, min_side):
    mat, _ = image_source(mat, single=f"{name} takes a single-channel image", max_side=FEATURE_MAX_SIDE)
    h, w = mat.shape
    if min(h, w) < min_side:
        raise ValueError(f"{name}: width and height must be at least {min_side}")
    if h * w > FEATURE_MAX_PIXELS:
        raise ValueError(f"{name}: more than 2^28 pixels are outside the accelerated path")
    return mat


def _image_call(mat, host_entry, dev_entry):
    """(ctx, entry, source pointer) of an operator whose results come back as host arrays whichever kind the image is"""
    ctx = _vp.default_context()
    if isinstance(mat, DeviceMat):
        mat.refresh_device(ctx)
        return ctx, dev_entry, mat.dev_ptr, mat
    mat = np.ascontiguousarray(mat)
    return ctx, host_entry, mat.ctypes.data, mat


def fast_corners(mat, threshold: int = 10, nonmax: bool = True, max_points=None):
    """cv2.FastFeatureDetector_create(threshold, nonmax, TYPE_9_16).detect on a uint8 single-channel image (numpy, or a DeviceMat that
    stays in HBM): (pts float32 (n, 2) of (x, y), scores int32 (n,)) in raster order - y, then x.  A pixel at least 3 from every border
    is a corner when nine contiguous pixels of its radius-3 ring are all brighter than it by more than `threshold`, or all darker; its
    score is the largest threshold at which it still is one.  nonmax keeps the corners whose score is strictly above that of all eight
    neighbours (two adjacent corners of equal score both go); without it every corner is kept and scores 0.  max_points keeps the
    highest scores, ties to the earlier raster position, and the result is in raster order again.  DESIGN.md section 4.31."""
    mat = _feature_image(mat, "fast_corners", FAST_MIN_SIDE)
    threshold = int(threshold)
    if not 0 <= threshold <= 255:
        raise ValueError("the threshold must be 0 to 255")
    if max_points is not None:
        max_points = int(max_points)
        if max_points < 0:
            raise ValueError("max_points must be at least 0")
    h, w = mat.shape
    lib = _vp.lib()
    ctx, entry, src, mat = _image_call(mat, lib.vp_fast_u8, lib.vp_fast_dev)
    cap = getattr(_fast_cap, "n", 4096)
    while True:
        xy, val = np.empty((max(cap, 1), 2), np.int32), np.empty(max(cap, 1), np.int32)
        n = _vp.C.c_int(0)
        _vp.check(entry(ctx.handle, src, w, w, h, threshold, int(bool(nonmax)), xy.ctypes.data, val.ctypes.data, cap, _vp.C.addressof(n)), ctx.handle)
        if n.value <= cap:
            break
        cap = _fast_cap.n = n.value                    # the true count came back: once more with room for all of them
    xy, val = xy[:n.value], val[:n.value]
    if max_points is not None and n.value > max_points:
        keep = np.sort(np.argsort(-val.astype(np.int64), kind="stable")[:max_points])
        xy, val = xy[keep], val[keep]
    return xy.astype(np.float32), val.copy()


def describe_points(mat, pts):
    """The library's 256-bit binary descriptor of the points `pts` ((N, 2) or (N, 1, 2), (x, y)) of a uint8 single-channel image (numpy,
    or a DeviceMat that stays in HBM): (kept_pts float32 (m, 2), desc uint8 (m, 32), kept_index (m,)).  A point is rounded to its
    pixel; points closer than 15 to a border, or not finite, are dropped, as cv2's `compute` drops them - kept_index says which stayed.
    Orientation: the intensity centroid over the disc of radius 15, quantised to 32 directions in integers; bits: 256 comparisons of
    the 7 x 7 Gaussian blur (sigma 2) at pattern points steered to that direction.  Not cv2.ORB's bits: the pattern is this library's
    (DESIGN.md section 4.31).  Tolerates in-plane rotation and small changes of scale; single scale."""
    mat = _feature_image(mat, "describe_points", DESCRIBE_MIN_SIDE)
    pts = _flow_points(pts, "the points")
    n = len(pts)
    if n > FEATURE_MAX_POINTS:
        raise ValueError("more than 1048576 points are outside the accelerated path")
    if n == 0:
        return np.empty((0, 2), np.float32), np.empty((0, DESCRIPTOR_BYTES), np.uint8), np.empty(0, np.intp)
    h, w = mat.shape
    lib = _vp.lib()
    ctx, entry, src, mat = _image_call(mat, lib.vp_describe_u8, lib.vp_describe_dev)
    desc, bins, status = np.empty((n, DESCRIPTOR_BYTES), np.uint8), np.empty(n, np.uint8), np.empty(n, np.uint8)
    _vp.check(entry(ctx.handle, src, w, w, h, pts.ctypes.data, n, desc.ctypes.data, bins.ctypes.data, status.ctypes.data), ctx.handle)
    keep = np.flatnonzero(status)
    return pts[keep], desc[keep], keep


def _descriptors(a, what):
    a = to_host_readonly(as_mat(a))
    if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 2:
        raise TypeError(f"{what} must be a uint8 (n, D) array")
    return a


def match_descriptors(query, train, k: int = 2, cross_check: bool = False):
    """cv2.BFMatcher(NORM_HAMMING, crossCheck).knnMatch(query, train, k) as arrays: (idx int32 (nq, k), dist int32 (nq, k)).  For each
    query row the train rows are ordered by (Hamming distance, index) and the first k taken; -1 / -1 where there are fewer than k.
    cross_check (k = 1): idx is -1 where the train row's own best query, by (distance, query index), is another one.  uint8 (n, D)
    arrays, D up to 128 bytes (rows are zero-padded to a multiple of 8, which leaves distances unchanged).  libvp vp_hamming_knn_u8."""
    query, train = as_mat(query), as_mat(train)
    on_device = (isinstance(query, DeviceMat) and isinstance(train, DeviceMat) and query.dtype == train.dtype == np.uint8 and query.ndim == train.ndim == 2
                 and query.shape[1] == train.shape[1] and query.shape[1] % 8 == 0)
    if not on_device:
        query, train = _descriptors(query, "the query descriptors"), _descriptors(train, "the train descriptors")
    k = int(k)
    if k not in (1, 2):
        raise ValueError("k must be 1 or 2")
    if cross_check and k != 1:
        raise ValueError("cross_check goes with k = 1")
    nq, nt = len(query), len(train)
    D = query.shape[1] if nq or not nt else train.shape[1]
    if nq and nt and train.shape[1] != D:
        raise ValueError("query and train descriptors must have the same length")
    if not 1 <= D <= HAMMING_MAX_BYTES:
        raise ValueError("descriptors of 1 to 128 bytes")
    if max(nq, nt) > HAMMING_MAX_ROWS:
        raise ValueError("more than 1048576 descriptors are outside the accelerated path")
    idx, dist = np.full((nq, k), -1, np.int32), np.full((nq, k), -1, np.int32)
    if nq == 0 or nt == 0:
        return idx, dist
    if on_device:
        return _match_descriptors_dev(query, train, k, cross_check)
    Dp = (D + 7) // 8 * 8

    def rows(a):
        if Dp == D:
            return np.ascontiguousarray(a)
        out = np.zeros((len(a), Dp), np.uint8)
        out[:, :D] = a
        return out
    q, t = rows(query), rows(train)
    ctx = _vp.default_context()
    _vp.check(_vp.lib().vp_hamming_knn_u8(ctx.handle, q.ctypes.data, Dp, nq, t.ctypes.data, Dp, nt, Dp, k, int(bool(cross_check)), idx.ctypes.data, dist.ctypes.data),
              ctx.handle)
    return idx, dist


def _match_descriptors_dev(query, train, k, cross_check):
    """match_descriptors of two DeviceMat arrays of the same row length, a multiple of 8 (what pyramid_features(device_descriptors=True)
    returns): libvp vp_hamming_knn_dev reads them where they are, and only the (nq, k) indices and distances come back."""
    ctx = _vp.default_context()
    query.refresh_device(ctx)
    train.refresh_device(ctx)
    nq, nt, D = len(query), len(train), query.shape[1]
    idx, dist = DeviceMat(ctx, (nq, k), np.int32), DeviceMat(ctx, (nq, k), np.int32)
    _vp.check(_vp.lib().vp_hamming_knn_dev(ctx.handle, query.dev_ptr, D, nq, train.dev_ptr, D, nt, D, k, int(bool(cross_check)), idx.dev_ptr, dist.dev_ptr), ctx.handle)
    return idx.host_copy(), dist.host_copy()


PYRAMID_MAX_LEVELS, PYRAMID_MAX_PIXELS = 8, 1 << 26


def pyramid_level_sizes(w: int, h: int, levels: int = 8):
    """The (w, h) of the pyramid levels pyramid_features builds on a w x h image: a step of 1.2 in integers, w_l = (5 w_{l-1} + 3) // 6,
    for as long as both sides are at least 31 and at most `levels` of them."""
    out = []
    while len(out) < levels and min(w, h) >= DESCRIBE_MIN_SIDE:
        out.append((w, h))
        w, h = (5 * w + 3) // 6, (5 * h + 3) // 6
    return out


def pyramid_features(mat, threshold: int = 20, max_points: int = 2000, levels: int = 8, device_descriptors: bool = False):
    """FAST-9 corners and the steered 256-bit descriptor of describe_points over a scale pyramid of a uint8 single-channel image (numpy,
    or a DeviceMat that stays in HBM): (pts0 float32 (n, 2), desc uint8 (n, 32), level int32 (n,), score int32 (n,), bin uint8 (n,)),
    n <= max_points, ordered by level, then y, then x.  Level l is the INTER_LINEAR resize of level l - 1 to (5 side + 3) // 6 - a step
    of 1.2 - and exists while both sides are at least 31, up to `levels` (1..8) of them; an image below 31 on a side gives no point.
    Each level keeps its share of max_points - in proportion to its area, level 0 taking the remainder - of its highest-scoring
    corners, ties to the earlier raster position.  A point is detected and described on its own level; pts0 are its coordinates in the
    image, ((x + 0.5) w_0 / w_l - 0.5 in double).  All levels are scored, selected and described by the same few launches, and the
    points never visit the host in between (libvp vp_pyr_features_*).  device_descriptors: desc is a DeviceMat,
    for match_descriptors between two of them."""
    mat, _ = image_source(mat, single="pyramid_features takes a single-channel image", max_side=FEATURE_MAX_SIDE)
    h, w = mat.shape
    if h * w > PYRAMID_MAX_PIXELS:
        raise ValueError("pyramid_features: more than 2^26 pixels are outside the accelerated path")
    threshold, max_points, levels = int(threshold), int(max_points), int(levels)
    if not 0 <= threshold <= 255:
        raise ValueError("the threshold must be 0 to 255")
    if not 0 <= max_points <= FEATURE_MAX_POINTS:
        raise ValueError("max_points must be 0 to 1048576")
    if not 1 <= levels <= PYRAMID_MAX_LEVELS:
        raise ValueError("levels must be 1 to 8")
    lib = _vp.lib()
    ctx, entry, src, mat = _image_call(mat, lib.vp_pyr_features_u8, lib.vp_pyr_features_dev)
    cap = max(max_points, 1)
    xy0, lxy, val = np.empty((cap, 2), np.float32), np.empty((cap, 3), np.int32), np.empty(cap, np.int32)
    bins, desc = np.empty(cap, np.uint8), np.empty((cap, DESCRIPTOR_BYTES), np.uint8)
    held = DeviceMat(ctx, (cap, DESCRIPTOR_BYTES), np.uint8) if device_descriptors else None
    n = _vp.C.c_int(0)
    _vp.check(entry(ctx.handle, src, w, w, h, levels, threshold, max_points, xy0.ctypes.data, lxy.ctypes.data, val.ctypes.data, bins.ctypes.data, desc.ctypes.data,
                    held.dev_ptr if held is not None else None, _vp.C.addressof(n)), ctx.handle)
    n = n.value
    out_desc = DeviceMat.over_buffer(ctx, held._buf, held._off, (n, DESCRIPTOR_BYTES), np.uint8) if held is not None else desc[:n].copy()
    return xy0[:n].copy(), out_desc, lxy[:n, 0].copy(), val[:n].copy(), bins[:n].copy()


def ratio_test(idx, dist, ratio: float = 0.7):
    """Lowe's ratio test on match_descriptors(k=2): (query indices, train indices) of the rows with dist[:, 0] < ratio * dist[:, 1] in
    float64.  Rows without a second neighbour are dropped."""
    idx, dist = np.asarray(idx), np.asarray(dist)
    if idx.ndim != 2 or idx.shape[1] != 2 or dist.shape != idx.shape:
        raise ValueError("the ratio test takes (n, 2) indices and distances")
    keep = (idx[:, 0] >= 0) & (idx[:, 1] >= 0) & (dist[:, 0].astype(np.float64) < float(ratio) * dist[:, 1].astype(np.float64))
    q = np.flatnonzero(keep)
    return q, idx[q, 0].astype(np.intp)


def hough_circles(mat, dp: float, min_dist: float, param1: float = 100, param2: float = 100, min_radius: int = 0, max_radius: int = 0):
    """cv2.HoughCircles(mat, cv2.HOUGH_GRADIENT, dp, min_dist, None, param1, param2, min_radius, max_radius) on the GPU (libvp
    vp_hough_circles_*): (1, N, 3) float32 (x, y, r) in cv2's order, or None when no circle is found.  A device image is read where it
    is.  max_radius < 0 (cv2's centres-only mode) is outside the accelerated path."""
    mat = as_mat(mat)
    ctx = _vp.default_context()
    if isinstance(mat, DeviceMat):
        if mat.dtype != np.uint8:
            raise TypeError("expected a uint8 single-channel image")
        src = device_image(ctx, mat, 1)
        h, w = src.shape
    else:
        if not isinstance(mat, np.ndarray) or mat.dtype != np.uint8:
            raise TypeError("expected a uint8 single-channel image")
        if mat.ndim == 3 and mat.shape[2] == 1:
            mat = mat[:, :, 0]
        if mat.ndim != 2 or mat.size == 0:
            raise ValueError("expected a non-empty (h, w) image")
        mat = np.ascontiguousarray(mat)
        h, w = mat.shape
        src = None
    args = (float(dp), float(min_dist), float(param1), float(param2), int(min_radius), int(max_radius))
    cap = getattr(_circles_cap, "n", 256)
    while True:
        out = np.empty((1, max(cap, 1), 3), np.float32)
        n = _vp.C.c_int(0)
        if src is not None:
            _vp.check(_vp.lib().vp_hough_circles_dev(ctx.handle, src.dev_ptr, w, w, h, *args, _vp.ptr(out), cap, _vp.C.byref(n)), ctx.handle)
        else:
            _vp.check(_vp.lib().vp_hough_circles_u8(ctx.handle, _vp.ptr(mat), w, h, *args, _vp.ptr(out), cap, _vp.C.byref(n)), ctx.handle)
        if n.value <= cap:
            break
        cap = _circles_cap.n = n.value                 # the true count came back: once more with room for all of them
    return out[:, :n.value].copy() if n.value else None


def hough_lines(mat, rho: float, theta: float, threshold: int, min_theta: float = 0.0, max_theta: float = np.pi):
    """cv2.HoughLines(mat, rho, theta, threshold, min_theta=min_theta, max_theta=max_theta) on the GPU (libvp vp_hough_lines_*):
    (N, 1, 2) float32 (rho, theta) in cv2's order, or None when no line is found.  A device image is read where it is."""
    mat = as_mat(mat)
    ctx = _vp.default_context()
    if isinstance(mat, DeviceMat):
        src = device_image(ctx, mat, 1)
        h, w = src.shape
    else:
        if not isinstance(mat, np.ndarray) or mat.dtype != np.uint8:
            raise TypeError("expected a uint8 single-channel image")
        if mat.ndim == 3 and mat.shape[2] == 1:
            mat = mat[:, :, 0]
        if mat.ndim != 2 or mat.size == 0:
            raise ValueError("expected a non-empty (h, w) image")
        mat = np.ascontiguousarray(mat)
        h, w = mat.shape
        src = None
    cap = getattr(_lines_cap, "n", 1024)
    while True:
        out = np.empty((max(cap, 1), 1, 2), np.float32)
        n = _vp.C.c_int(0)
        if src is not None:
            _vp.check(_vp.lib().vp_hough_lines_dev(ctx.handle, src.dev_ptr, w, w, h, float(rho), float(theta), int(threshold), float(min_theta),
                                                   float(max_theta), _vp.ptr(out), cap, _vp.C.byref(n)), ctx.handle)
        else:
            _vp.check(_vp.lib().vp_hough_lines_u8(ctx.handle, _vp.ptr(mat), w, h, float(rho), float(theta), int(threshold), float(min_theta),
                                                  float(max_theta), _vp.ptr(out), cap, _vp.C.byref(n)), ctx.handle)
        if n.value <= cap:
            break
        cap = _lines_cap.n = n.value                   # the true count came back: once more with room for all of them
    return out[:n.value].copy() if n.value else None


def line_polar_to_cartesian(rho: float, theta: float) -> Tuple[int, int, int, int]:
    """utils/feature.py:158-180: two points 1000 px either side of the foot of the normal.  The arithmetic stays in the dtype of the
    arguments (float32 for what find_lines returns), as in the reference, and int() truncates."""
    c, s = np.cos(theta), np.sin(theta)
    px, py = c * rho, s * rho
    return int(px + 1000 * (-s)), int(py + 1000 * c), int(px - 1000 * (-s)), int(py - 1000 * c)


def find_lines(mat: np.ndarray, rho: float, theta: float, threshold: int):
    """utils/feature.py:183-213 (cv2.HoughLines): (list of (x1, y1, x2, y2), list of (rho, theta) np.float32 pairs), strongest first."""
    lines = hough_lines(mat, rho, theta, threshold)
    cartesian, polar = [], []
    if lines is not None:
        for line in lines:
            r, t = line[0]
            cartesian.append(line_polar_to_cartesian(r, t))
            polar.append((r, t))
    return cartesian, polar


def find_contours(mat: np.ndarray, mode: int = _vp.RETR_EXTERNAL, method: int = _vp.CHAIN_APPROX_SIMPLE, with_holes: bool = False,
                  with_hierarchy: bool = False):
    """cv2.findContours(mat, mode, method)[0] on the GPU (libvp vp_find_contours_u8): tuple of (N,1,2) int32 arrays of
    (x, y) points, newest contour first like cv2.  with_hierarchy: also cv2's hierarchy, int32 (1, N, 4) rows [next, prev,
    first_child, parent] (None when there is no contour), through the vp_find_contours_tree_* entries, which take every mode
    (RETR_EXTERNAL, RETR_LIST, RETR_CCOMP, RETR_TREE); returned last: (contours, hierarchy) or (contours, holes, hierarchy)."""
    mat = as_mat(mat)
    ctx = _vp.default_context()
    dev = None
    if isinstance(mat, DeviceMat):                     # the mask is already in HBM (range_threshold / morphology result): read it there
        if mat.dtype != np.uint8:
            raise TypeError("expected a uint8 mask")
        dev = device_image(ctx, mat, 1)
        h, w = dev.shape
    else:
        if not isinstance(mat, np.ndarray) or mat.dtype != np.uint8:
            raise TypeError("expected a uint8 mask")
        if mat.ndim == 3 and mat.shape[2] == 1:
            mat = mat[:, :, 0]
        if mat.ndim != 2 or mat.size == 0:
            raise ValueError("expected a non-empty (h, w) mask")
        if mat.strides[1] != 1:
            mat = np.ascontiguousarray(mat)
        h, w = mat.shape
    # capacities that served the last call of this size: a mask with more contours than the first guess (speckle: modules/red_buoy.py:38
    # runs on the un-cleaned mask) would otherwise be traced twice at every call, once to learn the sizes and once to keep the result
    max_c, max_p, ttl = _capacity.get((h, w), (256, 1 << 14, 0))
    while True:
        # result arrays of the C call: per thread, kept from call to call (what is handed out below are copies of the used parts)
        sc = getattr(_scratch, "arrays", None)
        if sc is None or sc[0] != (max_c, max_p):
            pts = np.empty((max_p, 2), np.int32)
            counts = np.empty(max_c, np.int32)
            holes = np.empty(max_c, np.uint8)
            sc = _scratch.arrays = ((max_c, max_p), pts, counts, holes)
        _, pts, counts, holes = sc
        nc, npts = _vp.C.c_int32(0), _vp.C.c_int64(0)
        bits = dev.bit_plane(ctx) if dev is not None else None
        if with_hierarchy:
            hier = getattr(_scratch, "hier", None)
            if hier is None or len(hier) != max_c:
                hier = _scratch.hier = np.empty((max_c, 4), np.int32)
            if bits is not None and dev._dev_ok and dev._ctx is ctx:
                _vp.check(_vp.lib().vp_find_contours_tree_bits_dev(ctx.handle, bits.ptr, w, h, int(mode), int(method), _vp.ptr(pts), max_p,
                                                                   _vp.ptr(counts), _vp.ptr(holes), max_c, _vp.C.byref(nc), _vp.C.byref(npts),
                                                                   _vp.ptr(hier)), ctx.handle)
            elif dev is not None:
                _vp.check(_vp.lib().vp_find_contours_tree_dev(ctx.handle, dev.dev_ptr, w, w, h, int(mode), int(method), _vp.ptr(pts), max_p,
                                                              _vp.ptr(counts), _vp.ptr(holes), max_c, _vp.C.byref(nc), _vp.C.byref(npts),
                                                              _vp.ptr(hier)), ctx.handle)
            else:
                _vp.check(_vp.lib().vp_find_contours_tree_u8(ctx.handle, _vp.ptr(mat), mat.strides[0], w, h, int(mode), int(method), _vp.ptr(pts),
                                                             max_p, _vp.ptr(counts), _vp.ptr(holes), max_c, _vp.C.byref(nc), _vp.C.byref(npts),
                                                             _vp.ptr(hier)), ctx.handle)
        elif bits is not None and dev._dev_ok and dev._ctx is ctx:
            # the mask came with its bit plane (range_threshold) and has not been written to since: no packing launch
            _vp.check(_vp.lib().vp_find_contours_bits_dev(ctx.handle, bits.ptr, w, h, int(mode), int(method), _vp.ptr(pts), max_p,
                                                          _vp.ptr(counts), _vp.ptr(holes), max_c, _vp.C.byref(nc), _vp.C.byref(npts)), ctx.handle)
        elif dev is not None:
            _vp.check(_vp.lib().vp_find_contours_dev(ctx.handle, dev.dev_ptr, w, w, h, int(mode), int(method), _vp.ptr(pts), max_p,
                                                     _vp.ptr(counts), _vp.ptr(holes), max_c, _vp.C.byref(nc), _vp.C.byref(npts)), ctx.handle)
        else:
            _vp.check(_vp.lib().vp_find_contours_u8(ctx.handle, _vp.ptr(mat), mat.strides[0], w, h, int(mode), int(method), _vp.ptr(pts), max_p,
                                                    _vp.ptr(counts), _vp.ptr(holes), max_c, _vp.C.byref(nc), _vp.C.byref(npts)), ctx.handle)
        if nc.value <= max_c and npts.value <= max_p:
            break
        max_c = max(max_c, 2 * nc.value)
        max_p = max(max_p, 2 * npts.value)
    k = nc.value
    if k > 256 or npts.value > (1 << 14):
        _capacity[(h, w)] = (max(256, k + k // 2), max(1 << 14, npts.value + npts.value // 2), 32)     # follows the masks up and down ...
    elif ttl > 1:
        _capacity[(h, w)] = (max_c, max_p, ttl - 1)    # ... down only after 32 small results in a row: speckle that comes and goes is not traced twice each time
    else:
        _capacity.pop((h, w), None)
    flat = pts[:npts.value].copy()                     # one block for all contours; the arrays handed out are views of it
    if k > LazyContourList.THRESHOLD:
        out = LazyContourList(flat, counts[:k].copy())
    else:
        cnt = counts[:k].tolist()
        pts3 = flat.reshape(-1, 1, 2)
        out, o = [], 0
        for c in cnt:
            out.append(pts3[o:o + c])
            o += c
        out = ContourList(out)
        out._flat, out._counts = flat, counts[:k].copy()
    if with_hierarchy:
        hierarchy = hier[:k].reshape(1, k, 4).copy() if k else None
        return (out, holes[:k].copy(), hierarchy) if with_holes else (out, hierarchy)
    return (out, holes[:k].copy()) if with_holes else out


_capacity = {}            # (h, w) -> (contours, points, calls left before shrinking) the result arrays of find_contours start with
_scratch = threading.local()


class ContourList(tuple):
    """The tuple of (N, 1, 2) int32 arrays cv2.findContours returns.  The arrays are views of one point block (`_flat`, in the
    tuple's order), which `draw_contours` hands to the rasteriser as it is; writing to a contour writes to the block, so the two
    cannot disagree."""


class LazyContourList(_SequenceABC):
    """What find_contours returns for a mask with many contours (raw speckle: 17 k at 2 % noise): the same sequence of (N, 1, 2) views
    of one point block, made when they are looked at.  Building seventeen thousand array views up front took 2.2 ms of a 2.5 ms call;
    len(), indexing, slicing, iteration, `max(contours, key=...)` and the overlay (which reads the block itself) behave as on the tuple."""
    THRESHOLD = 512
    __slots__ = ("_flat", "_counts", "_ends", "_pts3")

    def __init__(self, flat, counts):
        self._flat, self._counts = flat, counts
        self._ends = np.cumsum(counts, dtype=np.int64)
        self._pts3 = flat.reshape(-1, 1, 2)

    def __len__(self):
        return len(self._counts)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return tuple(self[j] for j in range(*i.indices(len(self._counts))))
        n = len(self._counts)
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError("contour index out of range")
        e = int(self._ends[i])
        return self._pts3[e - int(self._counts[i]):e]

    def __iter__(self):
        pts3, o = self._pts3, 0
        for c in self._counts.tolist():
            yield pts3[o:o + c]
            o += c

    def __add__(self, other):
        return tuple(self) + tuple(other)

    def __radd__(self, other):
        return tuple(other) + tuple(self)

    def __repr__(self):
        return f"<{len(self)} contours, {len(self._flat)} points>"


def outer_contours(mat: np.ndarray) -> List[np.ndarray]:
    """utils/feature.py:5-21 (cv2.findContours RETR_EXTERNAL, CHAIN_APPROX_SIMPLE)."""
    return find_contours(mat, _vp.RETR_EXTERNAL, _vp.CHAIN_APPROX_SIMPLE)


def all_contours(mat: np.ndarray) -> List[np.ndarray]:
    """utils/feature.py:25-40 (cv2.findContours RETR_LIST, CHAIN_APPROX_SIMPLE)."""
    return find_contours(mat, _vp.RETR_LIST, _vp.CHAIN_APPROX_SIMPLE)
