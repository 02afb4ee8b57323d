"""Mirror of the reference utils/color.py for the hot path (same names, arguments, return structure).

Reference: utils/color.py:11-32 (`_convert_colorspace`: cv2.cvtColor + cv2.split), :105-121
(`range_threshold`: cv2.inRange), :66-103 (`thresh_color_distance`).  The arithmetic runs in libvp's
HIP kernels (include/vp.h: vp_cvt_color_u8, vp_inrange_u8, vp_inrange_f32, vp_color_distance_u8).
Returned arrays are fresh, writable, caller-owned numpy arrays, as with cv2.
"""
from math import sqrt
from typing import Callable, List, Tuple

import numpy as np

from vision import _vp
from vision.devmat import DeviceMat, finish_uploads, lazy_enabled, to_host
from vision.utils.helpers import as_mat, device_image, image_source, run_operator


def _u8_image(mat, channels):
    mat = to_host(as_mat(mat))
    if not isinstance(mat, np.ndarray) or mat.dtype != np.uint8:
        raise TypeError("expected a uint8 numpy image")
    if channels in (3, 4) and not (mat.ndim == 3 and mat.shape[2] == channels):
        raise ValueError(f"expected an (h, w, {channels}) image")
    if channels == 1:
        if mat.ndim == 3 and mat.shape[2] == 1:
            mat = mat[:, :, 0]
        if mat.ndim != 2:
            raise ValueError("expected an (h, w) image")
    if mat.shape[0] == 0 or mat.shape[1] == 0:
        raise ValueError("empty image")
    # rows must be dense; a row pitch is fine (views of wider images)
    if mat.strides[-1] != 1 or (mat.ndim == 3 and mat.strides[1] != mat.shape[2]) or mat.strides[0] < mat.shape[1] * (channels):
        mat = np.ascontiguousarray(mat)
    return mat


def _convert_colorspace(code: int) -> Callable[[np.ndarray], Tuple[np.ndarray, Tuple[np.ndarray, ...]]]:
    """utils/color.py:11-23: returns f(mat) -> (converted image, split channels)."""
    scn, dcn = _vp.CVT_CHANNELS.get(code, (3, 3))
    want_planes = code != _vp.HSV2BGR

    def _inner_device(mat):
        """The image stays in HBM: results are DeviceMat (vision/devmat.py), nothing is downloaded here."""
        ctx = _vp.default_context()
        up = []                                       # a host image is copied while the results are set up and the kernel is enqueued
        src = device_image(ctx, mat, 0 if scn == 4 else scn, pending=up)
        try:
            if scn == 4 and not (len(src.shape) == 3 and src.shape[2] == 4):
                raise ValueError("expected an (h, w, 4) image")
            h, w = src.shape[:2]
            conv = DeviceMat(ctx, (h, w) if dcn == 1 else (h, w, dcn))
            planes = [DeviceMat(ctx, (h, w)) for _ in range(dcn)] if (dcn == 3 and want_planes) else []
            arr = (_vp.C.c_void_p * 3)(*[p.dev_ptr for p in planes], *([None] * (3 - len(planes))))
            _vp.check(_vp.lib().vp_cvt_color_dev(ctx.handle, code, src.dev_ptr, w * scn, w, h, conv.dev_ptr, arr if planes else None), ctx.handle)
            if not want_planes:                           # HSV2BGR (colour-balance helper): channel copies are host views
                hc = conv.host(writable=False)
                return conv, tuple(np.ascontiguousarray(hc[:, :, c]) for c in range(3))
            if planes:
                return conv, tuple(planes)
            if dcn == 4:                                  # a 4-channel result comes without planes: cv2's split is a call of its own
                return conv, ()
            second = DeviceMat(ctx, (h, w))               # cv2.split of a single-channel image: a 1-tuple holding a copy
            _vp.check(_vp.lib().vp_cvt_color_dev(ctx.handle, code, src.dev_ptr, w * scn, w, h, second.dev_ptr, None), ctx.handle)
            return conv, (second,)
        finally:
            finish_uploads(ctx, up)                   # the caller's array may change from here on

    def _inner(mat: np.ndarray):
        mat = as_mat(mat)
        if lazy_enabled() or isinstance(mat, DeviceMat):
            return _inner_device(mat)
        mat = _u8_image(mat, scn)
        h, w = mat.shape[:2]
        conv = np.empty((h, w) if dcn == 1 else (h, w, dcn), np.uint8)
        planes = [np.empty((h, w), np.uint8) for _ in range(dcn)] if (dcn == 3 and want_planes) else []
        arr = (_vp.C.c_void_p * 3)(*[p.ctypes.data for p in planes], *([None] * (3 - len(planes))))
        ctx = _vp.default_context()
        _vp.check(_vp.lib().vp_cvt_color_u8(ctx.handle, code, _vp.ptr(mat), mat.strides[0], w, h, _vp.ptr(conv),
                                            arr if planes else None), ctx.handle)
        # cv2.split of a single-channel image returns a 1-tuple holding a copy
        if not want_planes:
            return conv, tuple(np.ascontiguousarray(conv[:, :, c]) for c in range(3))
        if dcn == 4:
            return conv, ()
        return conv, (tuple(planes) if planes else (conv.copy(),))
    return _inner


def _unsupported(name):
    def _inner(mat):
        raise NotImplementedError(f"{name}: conversion is outside the accelerated hot path")
    return _inner


bgr_to_lab = _convert_colorspace(_vp.BGR2LAB)
bgr_to_hsv = _convert_colorspace(_vp.BGR2HSV)
bgr_to_gray = _convert_colorspace(_vp.BGR2GRAY)
gray_to_bgr = _convert_colorspace(_vp.GRAY2BGR)
bgr_to_hls = _convert_colorspace(_vp.BGR2HLS)
bgr_to_ycrcb = _convert_colorspace(_vp.BGR2YCRCB)
bgr_to_luv = _unsupported("bgr_to_luv")
lab_to_bgr = _convert_colorspace(_vp.LAB2BGR)
hsv_to_bgr = _convert_colorspace(_vp.HSV2BGR)
# beyond the reference's name list (utils/color.py:26-28): the other conversions its modules ask cv2 for (vision_common.py:208-221)
bgr_to_yuv = _convert_colorspace(_vp.BGR2YUV)
yuv_to_bgr = _convert_colorspace(_vp.YUV2BGR)
bgr_to_xyz = _convert_colorspace(_vp.BGR2XYZ)
xyz_to_bgr = _convert_colorspace(_vp.XYZ2BGR)
ycrcb_to_bgr = _convert_colorspace(_vp.YCRCB2BGR)
hls_to_bgr = _convert_colorspace(_vp.HLS2BGR)


def bgr_to_lab_f32(mat: np.ndarray):
    """Extension: float32 BGR in [0,1] -> (lab float32 (h,w,3), (L, a, b) planes), analytic CIE L*a*b* (L 0..100)."""
    mat = np.ascontiguousarray(as_mat(mat), dtype=np.float32)
    if mat.ndim != 3 or mat.shape[2] != 3 or mat.size == 0:
        raise ValueError("expected a non-empty (h, w, 3) float image")
    h, w = mat.shape[:2]
    out = np.empty_like(mat)
    ctx = _vp.default_context()
    _vp.check(_vp.lib().vp_cvt_bgr2lab_f32(ctx.handle, _vp.ptr(mat), w, h, _vp.ptr(out)), ctx.handle)
    return out, tuple(np.ascontiguousarray(out[:, :, c]) for c in range(3))


def percentile_f32(arr: np.ndarray, q: float) -> float:
    """np.percentile(arr, q) (method 'linear') of a float32 array: the two neighbouring order statistics are selected on
    the GPU (libvp vp_order_stats_f32), the interpolation follows numpy's _lerp in float64."""
    flat = np.ascontiguousarray(arr, dtype=np.float32).ravel()
    n = flat.size
    if n == 0:
        raise ValueError("percentile of an empty array")
    virtual = (n - 1) * (float(q) / 100.0)
    lo = int(np.floor(virtual))
    lo = min(max(lo, 0), n - 1)
    gamma = virtual - lo
    a, b = _vp.C.c_float(), _vp.C.c_float()
    ctx = _vp.default_context()
    _vp.check(_vp.lib().vp_order_stats_f32(ctx.handle, _vp.ptr(flat), n, lo, _vp.C.byref(a), _vp.C.byref(b)), ctx.handle)
    a, b = np.float64(np.float32(a.value)), np.float64(np.float32(b.value))
    diff = b - a
    return float(b - diff * (1 - gamma)) if gamma >= 0.5 else float(a + diff * gamma)


def color_dist(c1, c2) -> float:
    """utils/color.py:35-48."""
    return sqrt((c1[0] - c2[0])**2 + (c1[1] - c2[1])**2 + (c1[2] - c2[2])**2)


def elementwise_color_dist(mat: np.ndarray, c) -> np.ndarray:
    """utils/color.py:51-63 (plain numpy in the reference too)."""
    return np.linalg.norm(as_mat(mat) - c, axis=2)


def _round_half_even(v):
    return int(np.rint(v))


def range_threshold(mat: np.ndarray, min, max) -> np.ndarray:
    """utils/color.py:105-121: cv2.inRange(mat, min, max) -> 0/255 mask.

    uint8 input with scalar or per-channel bounds (rounded half-to-even like cv2's scalar
    conversion), or float32 single-channel input (the `dists` image of thresh_color_distance)."""
    mat = as_mat(mat)
    ctx = _vp.default_context()
    if isinstance(mat, DeviceMat) and mat.dtype != np.uint8:
        mat = mat.host()
    if isinstance(mat, np.ndarray) and mat.dtype == np.float32:
        if mat.ndim == 3 and mat.shape[2] == 1:
            mat = mat[:, :, 0]
        if mat.ndim != 2:
            raise ValueError("float32 inRange supports single-channel images")
        if mat.strides[1] != 4:
            mat = np.ascontiguousarray(mat)
        h, w = mat.shape
        out = np.empty((h, w), np.uint8)
        lo = float(np.float32(np.ravel(min)[0] if np.ndim(min) else min))
        hi = float(np.float32(np.ravel(max)[0] if np.ndim(max) else max))
        _vp.check(_vp.lib().vp_inrange_f32(ctx.handle, _vp.ptr(mat), mat.strides[0], w, h, lo, hi, _vp.ptr(out)), ctx.handle)
        return out
    cn = 3 if (isinstance(mat, (np.ndarray, DeviceMat)) and mat.ndim == 3 and mat.shape[2] == 3) else 1
    on_device = lazy_enabled() or isinstance(mat, DeviceMat)
    up = []
    mat = device_image(ctx, mat, cn, pending=up) if on_device else _u8_image(mat, cn)
    h, w = mat.shape[:2]

    def bounds(b):
        if cn == 1 and type(b) in (int, float):          # the common call: Python numbers for one plane
            v = float(b)
            if -1e18 < v < 1e18:                         # (NaN and infinities take the general path below)
                r = round(v)                             # half to even, like np.rint (`min` / `max` are this function's parameters)
                return np.array([-2**31 if r < -2**31 else 2**31 - 1 if r > 2**31 - 1 else r], np.int32)
        b = np.atleast_1d(np.asarray(b, dtype=np.float64)).ravel()
        if b.size == 1 and cn == 3:
            b = np.array([b[0], 0.0, 0.0])  # cv2 scalar -> (v, 0, 0, 0)
        if b.size < cn:
            raise ValueError("bounds need one value per channel")
        return np.ascontiguousarray(np.clip(np.rint(b[:cn]), -2**31, 2**31 - 1).astype(np.int32))
    try:
        lo, hi = bounds(min), bounds(max)
    except BaseException:
        finish_uploads(ctx, up)
        raise
    if on_device:
        try:
            out = DeviceMat(ctx, (h, w), binary=True)
            if w % 64 == 0:
                # the mask's bit-packed form comes out of the same launch (1/8 B/px more): the contour pass of this very mask
                # (modules/red_buoy.py:38 outer_contours(threshed)) then needs no packing launch of its own
                from vision.devmat import _DevBuf
                bits = _DevBuf(ctx, h * (w // 64) * 8)
                made = _vp.C.c_int(0)
                _vp.check(_vp.lib().vp_inrange_u8_bits_dev(ctx.handle, mat.dev_ptr, w * cn, w, h, cn, _vp.ptr(lo), _vp.ptr(hi), out.dev_ptr, bits.ptr,
                                                          _vp.C.byref(made)), ctx.handle)
                if made.value:
                    out._bits = bits
                return out
            _vp.check(_vp.lib().vp_inrange_u8_dev(ctx.handle, mat.dev_ptr, w * cn, w, h, cn, _vp.ptr(lo), _vp.ptr(hi), out.dev_ptr), ctx.handle)
            return out
        finally:
            finish_uploads(ctx, up)
    out = np.empty((h, w), np.uint8)
    _vp.check(_vp.lib().vp_inrange_u8(ctx.handle, _vp.ptr(mat), mat.strides[0], w, h, cn, _vp.ptr(lo), _vp.ptr(hi), _vp.ptr(out)), ctx.handle)
    return out


def binary_threshold(mat: np.ndarray, threshold: int) -> np.ndarray:
    """utils/color.py:124-137 (cv2.threshold THRESH_BINARY on uint8): > threshold -> 255."""
    return range_threshold(mat, int(np.floor(threshold)) + 1, 255)


def binary_threshold_inv(mat: np.ndarray, threshold: int) -> np.ndarray:
    """utils/color.py:140-153: <= threshold -> 255."""
    return range_threshold(mat, 0, int(np.floor(threshold)))


def thresh_color_distance(split: List[np.ndarray], color, distance: float, auto_distance_percentile: float = None,
                          ignore_channels: List[int] = [], weights=(1, 1, 1)) -> Tuple[np.ndarray, np.ndarray]:
    """utils/color.py:66-103.  d2 = sum_i w_i * (float32(split_i) - color_i)^2 in float32 (numpy 1.x
    scalar semantics: the normalised float64 weight multiplies a float32 array as float32), mask =
    inRange(d2, 0, distance^2 [or the percentile]), second result uint8(sqrt(d2))."""
    weights_cp = list(weights)
    for idx in ignore_channels:
        weights_cp[idx] = 0
    weights_cp = np.asarray(weights_cp, dtype=np.float64) / np.linalg.norm(weights)
    planes = [_u8_image(p, 1) for p in split[:3]]
    h, w = planes[0].shape
    planes = [np.ascontiguousarray(p) for p in planes]
    skip = 0
    for i in range(3):
        if i in ignore_channels:
            skip |= 1 << i
    col = np.ascontiguousarray(np.asarray([color[0], color[1], color[2]], dtype=np.float32))
    wts = np.ascontiguousarray(weights_cp.astype(np.float32))
    d2 = np.empty((h, w), np.float32)
    sq = np.empty((h, w), np.uint8)
    arr = (_vp.C.c_void_p * 3)(*[p.ctypes.data for p in planes])
    ctx = _vp.default_context()
    _vp.check(_vp.lib().vp_color_distance_u8(ctx.handle, arr, w, h, _vp.ptr(col), _vp.ptr(wts), skip, _vp.ptr(d2), _vp.ptr(sq)), ctx.handle)
    if auto_distance_percentile:
        distance = min(percentile_f32(d2, auto_distance_percentile), distance**2)
    else:
        distance = distance**2
    return range_threshold(d2, 0, distance), sq


# the rest of the reference's utils/color.py (:156-392).  Every name of it is implemented here now: the thresholds, Otsu and the adaptive
# thresholds, kmeans with its two mask helpers (libvp vp_kmeans_*, vp_label_select_dev) and the white balances; only bgr_to_luv above
# still fails loudly instead of falling back to a CPU implementation


def _threshold(mat: np.ndarray, thresh: float, maxval: float, kind: int) -> np.ndarray:
    """cv2.threshold(mat, thresh, maxval, kind)[1] on uint8 images (libvp vp_threshold_u8; a DeviceMat gives a DeviceMat that stays in
    HBM, vp_threshold_u8_dev)."""
    mat = as_mat(mat)
    if isinstance(mat, DeviceMat):
        if mat.dtype != np.uint8 or mat.size == 0:
            raise TypeError("expected a non-empty uint8 numpy image")
        ctx = _vp.default_context()
        mat.refresh_device(ctx)
        # a BINARY / BINARY_INV result with maxval 255 is a 0 / 255 mask: morphology and contours take their bit paths on it
        mask = int(kind) in (_vp.THRESH_BINARY, _vp.THRESH_BINARY_INV) and mat.ndim == 2 and maxval == maxval and round(float(maxval)) == 255
        out = DeviceMat(ctx, mat.shape, binary=mask)
        _vp.check(_vp.lib().vp_threshold_u8_dev(ctx.handle, mat.dev_ptr, mat.size, float(thresh), float(maxval), int(kind), out.dev_ptr), ctx.handle)
        return out
    mat = to_host(mat)
    if not isinstance(mat, np.ndarray) or mat.dtype != np.uint8 or mat.size == 0:
        raise TypeError("expected a non-empty uint8 numpy image")
    mat = np.ascontiguousarray(mat)
    out = np.empty_like(mat)
    ctx = _vp.default_context()
    _vp.check(_vp.lib().vp_threshold_u8(ctx.handle, _vp.ptr(mat), mat.size, float(thresh), float(maxval), int(kind), _vp.ptr(out)), ctx.handle)
    return out


def max_threshold(mat: np.ndarray, threshold: float) -> np.ndarray:
    """utils/color.py:156-169 (THRESH_TRUNC): values above the threshold become the threshold."""
    return _threshold(mat, threshold, 0, 2)


def above_threshold(mat: np.ndarray, threshold: float) -> np.ndarray:
    """utils/color.py:172-185 (THRESH_TOZERO): values above the threshold are kept, the rest become zero."""
    return _threshold(mat, threshold, 0, 3)


def below_threshold(mat: np.ndarray, threshold: float) -> np.ndarray:
    """utils/color.py:188-199 (THRESH_TOZERO_INV): values above the threshold become zero, the rest are kept."""
    return _threshold(mat, threshold, 0, 4)



def otsu_threshold(mat: np.ndarray):
    """utils/color.py:204-217 (cv2.threshold(mat, 0, 255, THRESH_OTSU)): (threshold chosen by Otsu's method, thresholded image).  A
    DeviceMat gives a DeviceMat: histogram, scan and threshold run on the device (vp_otsu_threshold_dev) and only the 8 bytes of the
    chosen threshold come back."""
    return _otsu(mat, 255.0, 0)


def _otsu(mat, maxval: float, kind: int):
    mat = as_mat(mat)
    if isinstance(mat, DeviceMat):
        if mat.dtype != np.uint8:
            raise TypeError("expected a uint8 numpy image")
        from vision.devmat import _DevBuf
        ctx = _vp.default_context()
        src = device_image(ctx, mat, 1)
        h, w = src.shape
        mask = int(kind) in (_vp.THRESH_BINARY, _vp.THRESH_BINARY_INV) and round(float(maxval)) == 255
        out = DeviceMat(ctx, (h, w), binary=mask)
        word = _DevBuf(ctx, 8)
        _vp.check(_vp.lib().vp_otsu_threshold_dev(ctx.handle, src.dev_ptr, h * w, float(maxval), int(kind), word.ptr, out.dev_ptr), ctx.handle)
        t = _vp.C.c_double(0)
        _vp.check(_vp.lib().vp_memcpy_d2h(ctx.handle, _vp.C.addressof(t), word.ptr, 8), ctx.handle)
        return t.value, out
    mat = _u8_image(mat, 1)
    mat = np.ascontiguousarray(mat)
    out = np.empty_like(mat)
    t = _vp.C.c_double(0)
    ctx = _vp.default_context()
    _vp.check(_vp.lib().vp_otsu_threshold_u8(ctx.handle, _vp.ptr(mat), mat.size, float(maxval), int(kind), _vp.C.byref(t), _vp.ptr(out)), ctx.handle)
    return t.value, out



def _adaptive_mean(mat: np.ndarray, neighborhood_size: int, bias: float, kind: int, max_value: float = 255.0) -> np.ndarray:
    """libvp vp_adaptive_threshold_mean_u8: numpy in -> numpy out; a DeviceMat -> a DeviceMat that stays in HBM (_dev)."""
    mat = as_mat(mat)
    ctx = _vp.default_context()
    if isinstance(mat, DeviceMat):
        if mat.dtype != np.uint8:
            raise TypeError("expected a uint8 numpy image")
        src = device_image(ctx, mat, 1)
        h, w = src.shape
        dst = DeviceMat(ctx, (h, w), binary=float(max_value) == 255.0)
        _vp.check(_vp.lib().vp_adaptive_threshold_mean_dev(ctx.handle, src.dev_ptr, w, w, h, float(max_value), kind, int(neighborhood_size),
                                                           float(bias), dst.dev_ptr), ctx.handle)
        return dst
    mat = np.ascontiguousarray(_u8_image(mat, 1))
    out = np.empty_like(mat)
    _vp.check(_vp.lib().vp_adaptive_threshold_mean_u8(ctx.handle, _vp.ptr(mat), mat.shape[1], mat.shape[0], float(max_value), kind, int(neighborhood_size),
                                                      float(bias), _vp.ptr(out)), ctx.handle)
    return out


def adaptive_threshold_mean(mat: np.ndarray, neighborhood_size: int, bias: float = 0) -> np.ndarray:
    """utils/color.py:220-235 (cv2.adaptiveThreshold, ADAPTIVE_THRESH_MEAN_C, THRESH_BINARY): 255 where the pixel exceeds the mean of
    its neighbourhood minus the bias."""
    return _adaptive_mean(mat, neighborhood_size, bias, 0)


def adaptive_threshold_mean_inv(mat: np.ndarray, neighborhood_size: int, bias: float = 0) -> np.ndarray:
    """utils/color.py:238-254 (THRESH_BINARY_INV): 255 where the pixel does not exceed the mean of its neighbourhood minus the bias."""
    return _adaptive_mean(mat, neighborhood_size, bias, 1)


def _adaptive_gaussian(mat, neighborhood_size: int, bias: float, kind: int, max_value: float = 255.0):
    """libvp vp_adaptive_threshold_gaussian_u8 / _dev: numpy in -> numpy out; a DeviceMat (or the lazy mode) -> a DeviceMat that stays in
    HBM."""
    mat = as_mat(mat)
    ctx = _vp.default_context()
    if lazy_enabled() or isinstance(mat, DeviceMat):
        up = []
        src = device_image(ctx, mat, 1, pending=up)
        try:
            h, w = src.shape
            dst = DeviceMat(ctx, (h, w), binary=float(max_value) == 255.0)
            _vp.check(_vp.lib().vp_adaptive_threshold_gaussian_dev(ctx.handle, src.dev_ptr, w, w, h, float(max_value), kind, int(neighborhood_size),
                                                                   float(bias), dst.dev_ptr), ctx.handle)
        finally:
            finish_uploads(ctx, up)
        return dst
    mat = np.ascontiguousarray(_u8_image(mat, 1))
    out = np.empty_like(mat)
    _vp.check(_vp.lib().vp_adaptive_threshold_gaussian_u8(ctx.handle, _vp.ptr(mat), mat.shape[1], mat.shape[0], float(max_value), kind,
                                                          int(neighborhood_size), float(bias), _vp.ptr(out)), ctx.handle)
    return out


def adaptive_threshold_gaussian(mat: np.ndarray, neighborhood_size: int, bias: float = 0) -> np.ndarray:
    """utils/color.py:257-273 (cv2.adaptiveThreshold, ADAPTIVE_THRESH_GAUSSIAN_C, THRESH_BINARY): 255 where the pixel exceeds the
    Gaussian-weighted mean of its neighbourhood minus the bias (the exact mean of OpenCV's float32 taps, rounded half to even)."""
    return _adaptive_gaussian(mat, neighborhood_size, bias, 0)


def adaptive_threshold_gaussian_inv(mat: np.ndarray, neighborhood_size: int, bias: float = 0) -> np.ndarray:
    """utils/color.py:276-292 (THRESH_BINARY_INV): 255 where the pixel does not exceed the Gaussian-weighted mean minus the bias."""
    return _adaptive_gaussian(mat, neighborhood_size, bias, 1)


def _grey_source(mat):
    """The checked uint8 (h, w) source of equalize_hist and clahe, numpy or DeviceMat ((h, w, 1) comes back as (h, w)), in the words of
    _u8_image and device_image."""
    mat = as_mat(mat)
    if not isinstance(mat, (np.ndarray, DeviceMat)) or mat.dtype != np.uint8:
        raise TypeError("expected a uint8 numpy image")
    if mat.ndim == 3 and mat.shape[2] == 1:
        mat = mat.reshaped(mat.shape[:2]) if isinstance(mat, DeviceMat) else mat[:, :, 0]
    if mat.ndim != 2:
        raise ValueError("expected an (h, w) image")
    if mat.shape[0] == 0 or mat.shape[1] == 0:
        raise ValueError("empty image")
    return mat


def equalize_hist(mat: np.ndarray) -> np.ndarray:
    """cv2.equalizeHist on a uint8 (h, w) image (libvp vp_equalize_hist_u8 / _dev).  An addition to the mirror, not a name of the
    reference's utils/color.py: the global contrast step.  Integer histogram, one float32 multiply per table entry, a table: byte for
    byte OpenCV's result.  numpy in gives numpy out; a DeviceMat gives a DeviceMat and stays in HBM (three launches, no wait)."""
    mat = _grey_source(mat)
    h, w = mat.shape
    lib = _vp.lib()
    return run_operator(mat, (h, w), np.uint8, lambda ctx, s, d: lib.vp_equalize_hist_u8(ctx.handle, s, w, h, d),
                        lambda ctx, s, d: lib.vp_equalize_hist_dev(ctx.handle, s, w, w, h, d))


def _clahe_params(clip_limit, tile_grid):
    try:
        clip, (tx, ty) = float(clip_limit), (int(tile_grid[0]), int(tile_grid[1]))
    except (TypeError, ValueError, IndexError):
        raise ValueError("clip_limit must be a number and tile_grid a pair of integers") from None
    if clip != clip or tx < 1 or ty < 1:
        raise ValueError("clip_limit must not be NaN and tile_grid must be at least (1, 1)")
    return clip, tx, ty


def clahe(mat: np.ndarray, clip_limit: float = 2.0, tile_grid=(8, 8)) -> np.ndarray:
    """cv2.createCLAHE(clip_limit, tile_grid).apply(mat) on a uint8 (h, w) image (libvp vp_clahe_u8 / _dev).  An addition to the mirror,
    not a name of the reference's utils/color.py: contrast-limited adaptive histogram equalisation, the usual first step on underwater
    frames.  tile_grid is (tiles_x, tiles_y) as in cv2, up to 64 each.  Byte for byte OpenCV's result, including its padding of images
    that the grid does not divide.  numpy in gives numpy out; a DeviceMat gives a DeviceMat and stays in HBM."""
    clip, tx, ty = _clahe_params(clip_limit, tile_grid)
    mat = _grey_source(mat)
    h, w = mat.shape
    lib = _vp.lib()
    return run_operator(mat, (h, w), np.uint8, lambda ctx, s, d: lib.vp_clahe_u8(ctx.handle, s, w, h, clip, tx, ty, d),
                        lambda ctx, s, d: lib.vp_clahe_dev(ctx.handle, s, w, w, h, clip, tx, ty, d))


def clahe_bgr(mat: np.ndarray, clip_limit: float = 2.0, tile_grid=(8, 8)) -> np.ndarray:
    """CLAHE of the L channel of a BGR image: bgr_to_lab -> split -> clahe(L) -> merge -> lab_to_bgr, each step the operator of that name.
    An addition to the mirror.  A DeviceMat gives a DeviceMat, and no step visits the host; a numpy image gives what bgr_to_lab gives for
    one (device images in the lazy mode, numpy otherwise)."""
    from vision import cv2_facade
    _clahe_params(clip_limit, tile_grid)
    _lab, (l, a, b) = bgr_to_lab(mat)
    return lab_to_bgr(cv2_facade.merge((clahe(l, clip_limit, tile_grid), a, b)))[0]


# ---- colour k-means (libvp vp_kmeans.hip) ------------------------------------------------------------------------
KMEANS_MAX_SIDE, KMEANS_MAX_K, KMEANS_MAX_ITER = 4096, 256, 100


def kmeans_seed_indices(n: int, k: int, seed: int) -> np.ndarray:
    """The k distinct raster indices of the initial centres of a seeded run: drawn without replacement from
    np.random.default_rng(seed), sorted, int32."""
    return np.sort(np.random.default_rng(seed).choice(n, size=k, replace=False)).astype(np.int32)


def kmeans_run(mat, k: int, max_iter: int, eps: float, centers=None, seed_index=None, labels=True):
    """One run of libvp's vp_kmeans_* on a uint8 image, (h, w) or (h, w, 1..4): (compactness, labels, centres (k, cn) float32, counts
    (k,) uint32, assign passes).  The initial centres are `centers` (k x cn values) or the pixels at the raster indices `seed_index`.
    A DeviceMat (or the lazy mode) is clustered where it is and gives int32 labels that stay in HBM; labels=False asks for the
    statistics alone (None in their place)."""
    mat, cn = image_source(mat)
    h, w = mat.shape[:2]
    k, max_iter, eps = int(k), int(max_iter), float(eps)
    if max(h, w) > KMEANS_MAX_SIDE:
        raise ValueError("sides above 4096 are outside the accelerated path")
    if not 1 <= k <= KMEANS_MAX_K:
        raise ValueError("the number of centres must be in 1..256")
    if k > h * w:
        raise ValueError("more centres than pixels")
    if not 1 <= max_iter <= KMEANS_MAX_ITER:
        raise ValueError("the iterations must be in 1..100")
    if not (eps >= 0.0 and np.isfinite(eps)):
        raise ValueError("epsilon must be finite and not negative")
    if (centers is None) == (seed_index is None):
        raise ValueError("exactly one of centers and seed_index must be given")
    if centers is not None:
        init = np.ascontiguousarray(np.asarray(centers, dtype=np.float32).reshape(-1))
        if init.size != k * cn or not np.isfinite(init).all():
            raise ValueError("the initial centres must be k x channels finite values")
        cptr, sptr = init.ctypes.data, None
    else:
        init = np.ascontiguousarray(np.asarray(seed_index).reshape(-1).astype(np.int64))
        if init.size != k or init.min() < 0 or init.max() >= h * w:
            raise ValueError("the seed indices must be k raster indices of the image")
        init = init.astype(np.int32)
        cptr, sptr = None, init.ctypes.data
    out = np.zeros(16 + 4 * k * cn + 4 * k, np.uint8)
    ctx = _vp.default_context()
    lib = _vp.lib()
    if lazy_enabled() or isinstance(mat, DeviceMat):
        up = []
        try:
            if isinstance(mat, DeviceMat):
                mat.refresh_device(ctx)
            else:
                mat = DeviceMat.from_host(ctx, mat, pending=up)
            lab = DeviceMat(ctx, (h, w), np.int32) if labels else None
            _vp.check(lib.vp_kmeans_dev(ctx.handle, mat.dev_ptr, w * cn, w, h, cn, k, cptr, sptr, max_iter, eps, None if lab is None else lab.dev_ptr, w * 4,
                                        out.ctypes.data), ctx.handle)
        finally:
            finish_uploads(ctx, up)
    else:
        mat = np.ascontiguousarray(mat)
        lab = np.empty((h, w), np.int32) if labels else None
        _vp.check(lib.vp_kmeans_u8(ctx.handle, mat.ctypes.data, w, h, cn, k, cptr, sptr, max_iter, eps, None if lab is None else lab.ctypes.data,
                                   out.ctypes.data), ctx.handle)
    compactness = float(out[:8].view(np.float64)[0])
    passes = int(out[8:12].view(np.int32)[0])
    centres = out[16:16 + 4 * k * cn].view(np.float32).reshape(k, cn).copy()
    counts = out[16 + 4 * k * cn:].view(np.uint32).copy()
    return compactness, lab, centres, counts, passes


def kmeans(mat: np.ndarray, num_centeroids: int, iterations: int = 10, epsilon: float = 1.0, *, centers=None, seed: int = 0,
           attempts: int = 1) -> Tuple[float, np.ndarray, np.ndarray]:
    """utils/color.py:295-323 as it was meant (the reference body cannot run: it reshapes to (-1, 2), calls np.reshape without an array
    and hard-codes 10 iterations and epsilon 1.0 whatever it is given): clusters the colours of a uint8 image, (h, w) or (h, w, 1..4),
    around num_centeroids centres on the GPU and returns (compactness, labels (h, w) int32, centers (k, channels) float32).
    `iterations` (1..100) and `epsilon` are honoured.  What is computed is stated in DESIGN.md section 4.26 and tests/kmeans_restate.py;
    it is what cv2.kmeans approximates, not its bits: distances in double, ties to the lowest index, exact integer sums, and an empty
    cluster keeps its centre where OpenCV re-seeds it.

    Additions to the mirror: `centers`, k x channels initial centres; without it the initial centres are num_centeroids distinct pixels
    drawn from np.random.default_rng(seed + attempt), sorted by raster index and gathered on the device.  With attempts > 1 the run with
    the smallest compactness wins, the first one on ties.  A DeviceMat in, or the lazy mode, gives a DeviceMat of labels that stays
    in HBM; numpy in otherwise gives numpy out."""
    attempts = int(attempts)
    if attempts < 1:
        raise ValueError("attempts must be at least 1")
    mat, _cn = image_source(mat)
    n, k = mat.shape[0] * mat.shape[1], int(num_centeroids)
    if not 1 <= k <= min(n, KMEANS_MAX_K):
        raise ValueError("the number of centres must be in 1..256 and at most the number of pixels")
    if centers is not None:
        return kmeans_run(mat, k, iterations, epsilon, centers=centers)[:3]
    best = None
    for attempt in range(attempts):
        run = kmeans_run(mat, k, iterations, epsilon, seed_index=kmeans_seed_indices(n, k, int(seed) + attempt))
        if best is None or run[0] < best[0]:
            best = run
    return best[0], best[1], best[2]


def _label_mask(ctx, labels: DeviceMat, select: np.ndarray) -> DeviceMat:
    """libvp vp_label_select_dev: the 0 / 255 mask of the labels whose byte in `select` is set, with its bit plane where the width
    allows (as range_threshold's masks carry one)."""
    from vision.devmat import _DevBuf
    h, w = labels.shape
    out = DeviceMat(ctx, (h, w), binary=True)
    bits = _DevBuf(ctx, h * (w // 64) * 8) if w % 64 == 0 else None
    _vp.check(_vp.lib().vp_label_select_dev(ctx.handle, labels.dev_ptr, w * 4, w, h, select.ctypes.data, len(select), out.dev_ptr, w,
                                            None if bits is None else bits.ptr), ctx.handle)
    out._bits = bits
    return out


def _device_labels(labels, centers):
    """the context when `labels` is a device label image vp_label_select_dev takes for these centres, else None"""
    if not (isinstance(labels, DeviceMat) and labels.dtype == np.int32 and labels.ndim == 2 and 1 <= len(centers) <= KMEANS_MAX_K
            and 0 not in labels.shape and max(labels.shape) <= KMEANS_MAX_SIDE):
        return None
    ctx = _vp.default_context()
    labels.refresh_device(ctx)
    return ctx


def mask_from_labels(labels: np.ndarray, centers: np.ndarray) -> List[np.ndarray]:
    """utils/color.py:326-345: one 0 / 255 mask per centre.  numpy labels: plain numpy, as in the reference.  The DeviceMat of labels
    that kmeans returns: one mask per centre on the device (libvp vp_label_select_dev), each a DeviceMat known to be binary that
    carries its bit plane when the width is a multiple of 64, so erode, distance_transform or median_blur read it packed."""
    ctx = _device_labels(labels, centers)
    if ctx is not None:
        return [_label_mask(ctx, labels, (np.arange(len(centers)) == i).astype(np.uint8)) for i in range(len(centers))]
    acc = []
    for i, _c in enumerate(centers):
        mask = np.zeros(labels.shape, dtype=np.uint8)
        mask[labels == i] = 255
        acc.append(mask)
    return acc


def mask_from_labels_target_color(labels: np.ndarray, centers: np.ndarray, target_color, distance_func: Callable = color_dist) -> np.ndarray:
    """utils/color.py:347-368 as it was meant: the 0 / 255 mask of the cluster whose centre is nearest to target_color, by
    distance_func(centre, target_color), the lowest index on ties.  The reference hands the (index, centre) tuple of enumerate() to
    distance_func and compares the labels with that tuple, which is a bug: its mask is always empty.  A DeviceMat of labels gives a
    DeviceMat (see mask_from_labels)."""
    if len(centers) == 0:
        raise ValueError("no centres")
    dists = [distance_func(c, target_color) for c in centers]
    target = min(range(len(dists)), key=lambda i: dists[i])          # min keeps the first of equal keys
    ctx = _device_labels(labels, centers)
    if ctx is not None:
        return _label_mask(ctx, labels, (np.arange(len(centers)) == target).astype(np.uint8))
    ret = np.zeros(labels.shape, dtype=np.uint8)
    ret[labels == target] = 255
    return ret


def _white_balance(bgr_img, kernel_size, ab_mean_out=None):
    """libvp vp_white_balance_u8 / _dev: numpy in -> numpy out; a DeviceMat (or the lazy mode) -> a DeviceMat that stays in HBM."""
    mat = as_mat(bgr_img)
    out_mean = np.zeros(2, np.float32) if ab_mean_out is not None else None
    ctx = _vp.default_context()
    if lazy_enabled() or isinstance(mat, DeviceMat):
        up = []
        src = device_image(ctx, mat, 3, pending=up)
        try:
            h, w = src.shape[:2]
            dst = DeviceMat(ctx, (h, w, 3))
            _vp.check(_vp.lib().vp_white_balance_dev(ctx.handle, src.dev_ptr, w * 3, w, h, int(kernel_size), dst.dev_ptr, _vp.ptr(out_mean)),
                      ctx.handle)
        finally:
            finish_uploads(ctx, up)
    else:
        mat = _u8_image(mat, 3)
        h, w = mat.shape[:2]
        dst = np.empty((h, w, 3), np.uint8)
        _vp.check(_vp.lib().vp_white_balance_u8(ctx.handle, _vp.ptr(mat), mat.strides[0], w, h, int(kernel_size), _vp.ptr(dst),
                                                _vp.ptr(out_mean)), ctx.handle)
    if ab_mean_out is not None:
        ab_mean_out[:] = out_mean
    return dst


def white_balance_bgr(bgr_img, ab_mean_out=None):
    """utils/color.py:370-378: a and b of the 8-bit Lab image moved so that their means (np.mean of the float32 planes) become 128,
    cast back with numpy's astype(np.uint8) (truncation, low 8 bits), LAB2BGR.  ab_mean_out (optional float32[2]) receives the means."""
    return _white_balance(bgr_img, _vp.WB_GLOBAL_MEAN, ab_mean_out)


def white_balance_bgr_blur(bgr_img, kernel_size):
    """utils/color.py:381-392: as white_balance_bgr with the k x k box mean (cv2.blur, BORDER_REPLICATE) in place of the global mean,
    k = 2 * (kernel_size // 2) + 1; a negative kernel_size raises the facade's cv2.error (vision.cv2_facade.error), as cv2.blur does."""
    k = 2 * (int(kernel_size) // 2) + 1
    if k <= 0:                                    # the reference fails inside cv2.blur with cv2.error
        from vision.cv2_facade import error
        raise error(f"white_balance_bgr_blur: kernel size {k} is not positive")
    return _white_balance(bgr_img, k)


# ---- colour-histogram tracking (libvp vp_hist.hip) ---------------------------------------------------------------
HIST_MAX_SIDE, HIST_MAX_DIMS, HIST_MAX_SIZE = 4096, 3, 256


class _HistDesc:
    """The checked description of a histogram: dims, channel indices, sizes and (low, high) ranges as the arrays libvp reads.
    Everything the C entries refuse about a description is refused here, before a device is needed."""
    __slots__ = ("dims", "channels", "sizes", "ranges", "shape")

    def __init__(self, cn, channels, hist_size, ranges):
        try:
            channels = [int(c) for c in np.asarray(channels).reshape(-1)]
            sizes = [int(s) for s in np.asarray(hist_size).reshape(-1)]
            flat = [float(r) for r in np.asarray(ranges, dtype=np.float64).reshape(-1)]
        except (TypeError, ValueError):
            raise ValueError("channels, sizes and ranges must be lists of numbers; non-uniform ranges are outside the accelerated path") from None
        dims = len(channels)
        if not 1 <= dims <= HIST_MAX_DIMS:
            raise ValueError("a histogram has 1 to 3 dimensions")
        if len(sizes) != dims:
            raise ValueError("one histogram size per dimension")
        if len(flat) != 2 * dims:
            raise ValueError("one (low, high) pair per dimension: non-uniform ranges are outside the accelerated path")
        if any(c < 0 or c >= cn for c in channels):
            raise ValueError("a channel index is outside the image's channels")
        if any(not 1 <= s <= HIST_MAX_SIZE for s in sizes):
            raise ValueError("a histogram size must be 1 to 256")
        if any(not (np.isfinite(flat[2 * d]) and np.isfinite(flat[2 * d + 1]) and flat[2 * d] < flat[2 * d + 1]) for d in range(dims)):
            raise ValueError("a range needs finite ends with low < high")
        self.dims, self.shape = dims, tuple(sizes)
        self.channels, self.sizes, self.ranges = np.array(channels, np.int32), np.array(sizes, np.int32), np.array(flat, np.float64)

    def args(self):
        return self.dims, self.channels.ctypes.data, self.sizes.ctypes.data, self.ranges.ctypes.data


def _hist_source(mat):
    """(image or DeviceCrop, channels, w, h)"""
    from vision.utils.feature import DeviceCrop
    if isinstance(mat, DeviceCrop):
        return mat, (1 if mat.mat.ndim == 2 else mat.mat.shape[2]), mat.w, mat.h
    mat, cn = image_source(mat, max_side=HIST_MAX_SIDE)
    return mat, cn, mat.shape[1], mat.shape[0]


def _hist_mask(mask, w, h):
    if mask is None:
        return None
    mask, _ = image_source(mask, single="the mask must be a single-channel image",
                           said=("the mask must be uint8", "the mask must be a non-empty (h, w) image", None))
    if tuple(mask.shape) != (h, w):
        raise ValueError("the mask must have the size of the image")
    return mask


def color_histogram(mat, channels, hist_size, ranges, mask=None) -> np.ndarray:
    """cv2.calcHist of one uint8 image of 1..4 channels: the float32 histogram of 1..3 dimensions over the
    given channel indices, `hist_size` uniform bins per dimension over ranges = [low0, high0, low1, high1, ...], the upper ends
    exclusive.  mask (uint8, the image's size): only its non-zero pixels are counted.  The counts are exact integers, counted on the
    GPU (libvp vp_calc_hist_*): a DeviceMat - or a DeviceCrop, the window of one - is read where it is, a device mask that still
    carries its bit plane through that, and only the counts come back."""
    from vision.utils.feature import DeviceCrop
    mat, cn, w, h = _hist_source(mat)
    desc = _HistDesc(cn, channels, hist_size, ranges)
    mask = _hist_mask(mask, w, h)
    ctx = _vp.default_context()
    lib = _vp.lib()
    if not isinstance(mat, (DeviceMat, DeviceCrop)):
        mat = np.ascontiguousarray(mat)
        out = np.empty(desc.shape, np.float32)
        m = None if mask is None else np.ascontiguousarray(to_host(mask) if isinstance(mask, DeviceMat) else mask)
        _vp.check(lib.vp_calc_hist_u8(ctx.handle, mat.ctypes.data, w, h, cn, *desc.args(), None if m is None else m.ctypes.data, w if m is not None else 0,
                                      h if m is not None else 0, out.ctypes.data), ctx.handle)
        return out
    if isinstance(mat, DeviceCrop):
        mat.mat.refresh_device(ctx)
        full_w = mat.mat.shape[1]
        ptr, stride = mat.mat.dev_ptr + (mat.y * full_w + mat.x) * cn, full_w * cn
    else:
        mat.refresh_device(ctx)
        ptr, stride = mat.dev_ptr, w * cn
    mp = bp = None
    if mask is not None:
        mask = device_image(ctx, mask, 1)
        mp = mask.dev_ptr
        if mask.binary:
            bits = mask.bit_plane(ctx)
            bp = bits.ptr if (bits is not None and mask._dev_ok and mask._ctx is ctx) else None
    counts = np.empty(desc.shape, np.uint32)
    _vp.check(lib.vp_calc_hist_dev(ctx.handle, ptr, stride, w, h, cn, *desc.args(), mp, w, w if mask is not None else 0, h if mask is not None else 0, bp,
                                   None, counts.ctypes.data), ctx.handle)
    return counts.astype(np.float32)              # exact: a count is at most 2^24


def normalize_hist(hist, top: float = 255.0, low: float = 0.0) -> np.ndarray:
    """The min-max stretch of a float32 array onto [low, top]: float32(low + (double(v) - min) * ((top - low) / (max - min))), one
    rounding; all `low` when max == min.  This library's own arithmetic: cv2.normalize(NORM_MINMAX) computes the same in float32 steps."""
    hist = np.asarray(hist)
    if hist.dtype != np.float32 or hist.size == 0 or not np.isfinite(hist).all():
        raise ValueError("expected a non-empty float32 array of finite values")
    top, low = float(top), float(low)
    if not (np.isfinite(top) and np.isfinite(low)):
        raise ValueError("the ends of the stretch must be finite")
    v = hist.astype(np.float64)
    lo, hi = v.min(), v.max()
    if not hi > lo:
        return np.full(hist.shape, low, np.float64).astype(np.float32)
    return (low + (v - lo) * ((top - low) / (hi - lo))).astype(np.float32)


def fold_hist(hist, scale: float = 1.0) -> np.ndarray:
    """The byte table of a back-projection: saturate_u8(round_half_even(double(hist) * scale)) per bin (a NaN product gives 0) - what
    libvp's fold computes, here for a histogram that is on the host."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(np.asarray(hist, dtype=np.float32).astype(np.float64) * float(scale))
    out = np.zeros(r.shape, np.uint8)
    pos = r > 0
    out[pos] = np.minimum(r[pos], 255.0).astype(np.uint8)
    return out


def _checked_hist(hist, desc):
    hist = to_host(hist) if isinstance(hist, DeviceMat) else np.asarray(hist)
    if hist.dtype != np.float32:
        raise TypeError("the histogram must be float32")
    if hist.ndim == desc.dims + 1 and hist.shape[-1] == 1:
        hist = hist.reshape(hist.shape[:-1])
    if tuple(hist.shape) != desc.shape:
        raise ValueError("the histogram's shape must be the histogram sizes (sparse histograms are outside the accelerated path)")
    return np.ascontiguousarray(hist)


def back_project(mat, channels, hist, ranges, scale: float = 1.0):
    """cv2.calcBackProject of one uint8 image of 1..4 channels: every pixel becomes
    saturate_u8(round_half_even(double(hist[bin]) * scale)) of its bin in the float32 histogram `hist` (its shape gives the sizes), 0
    when it falls into none.  numpy in gives numpy out; a DeviceMat gives a DeviceMat that stays in HBM (libvp vp_back_project_*): the
    histogram is folded into a byte table on the device and the image gathers from it."""
    mat, cn = image_source(mat, max_side=HIST_MAX_SIDE)
    h, w = mat.shape[:2]
    hshape = np.shape(hist)
    nd = len(np.asarray(channels).reshape(-1))
    desc = _HistDesc(cn, channels, hshape[:nd], ranges)
    hist = _checked_hist(hist, desc)
    scale = float(scale)
    if not np.isfinite(scale):
        raise ValueError("the scale must be finite")
    lib = _vp.lib()

    def on_device(ctx, s, d):
        held = DeviceMat.from_host(ctx, hist)                # (lives until the call is queued)
        return lib.vp_back_project_dev(ctx.handle, s, w * cn, w, h, cn, *desc.args(), held.dev_ptr, scale, d, w)

    return run_operator(mat, (h, w), np.uint8, lambda ctx, s, d: lib.vp_back_project_u8(ctx.handle, s, w, h, cn, *desc.args(), hist.ctypes.data, scale, d),
                        on_device)


class HistModel:
    """A colour model kept in HBM: the folded byte table of a histogram with its channels and ranges, as RemapTable holds a
    calibration's maps.  `apply` back-projects a frame with one launch and no synchronisation (libvp vp_back_project_table_dev)."""
    __slots__ = ("channels", "hist_size", "ranges", "hist", "table")

    def __init__(self, hist, channels, ranges, scale: float = 1.0):
        nd = len(np.asarray(channels).reshape(-1))
        desc = _HistDesc(4, channels, np.shape(hist)[:nd], ranges)      # (the channel indices are checked against each frame)
        self.hist = _checked_hist(hist, desc)
        self.channels, self.hist_size, self.ranges = tuple(int(c) for c in desc.channels), desc.shape, tuple(float(r) for r in desc.ranges)
        self.table = DeviceMat.from_host(_vp.default_context(), fold_hist(self.hist, scale))

    @classmethod
    def from_patch(cls, mat, channels, hist_size, ranges, mask=None, top: float = 255.0):
        """The model of a sample patch - an image, or a DeviceCrop of a frame in HBM: its histogram, stretched onto [0, top]
        (normalize_hist)."""
        return cls(normalize_hist(color_histogram(mat, channels, hist_size, ranges, mask), top), channels, ranges)

    def apply(self, mat):
        """The back-projection of the model onto a frame: a DeviceMat gives a DeviceMat, numpy gives numpy."""
        mat, cn = image_source(mat, max_side=HIST_MAX_SIDE)
        desc = _HistDesc(cn, self.channels, self.hist_size, self.ranges)
        h, w = mat.shape[:2]
        ctx = _vp.default_context()
        src = device_image(ctx, mat, 0)
        self.table.refresh_device(ctx)
        out = DeviceMat(ctx, (h, w), np.uint8)
        _vp.check(_vp.lib().vp_back_project_table_dev(ctx.handle, src.dev_ptr, w * cn, w, h, cn, *desc.args(), self.table.dev_ptr, out.dev_ptr, w), ctx.handle)
        return out if isinstance(mat, DeviceMat) else out.host_copy()
