"""Mirror of the reference utils/transform.py for the hot path.

Reference: utils/transform.py:27-77 (`elliptic_kernel`, `rect_kernel`), :80-112 (`erode`, `dilate`),
:115-164 (`morph_remove_noise`, `morph_close_holes`, `morph_borders`).  Kernels: libvp vp_morph_u8
(bit-plane LDS stencils for 0/255 masks with rect kernels, generic kernel otherwise).
"""
from typing import Optional

import numpy as np

from vision import _vp
from vision.devmat import DeviceMat, defer_enabled, lazy_enabled
from vision.utils.helpers import as_mat, device_image


def _structuring_element(shape, x, y):
    out = np.empty((y, x), np.uint8)
    _vp.check(_vp.lib().vp_structuring_element(shape, x, y, _vp.ptr(out)))
    return out


def elliptic_kernel(x: int, y: Optional[int] = None) -> np.ndarray:
    """utils/transform.py:27-51: odd positive sizes only (ValueError otherwise)."""
    if y is None:
        y = x
    if x % 2 == 0 or y % 2 == 0 or x <= 0 or y <= 0:
        raise ValueError("x and y must be odd positive integers")
    return _structuring_element(_vp.SHAPE_ELLIPSE, int(x), int(y))


def rect_kernel(x: int, y: Optional[int] = None) -> np.ndarray:
    """utils/transform.py:54-77."""
    if y is None:
        y = x
    if x <= 0 or y <= 0:
        raise ValueError("x and y must be positive integers")
    return _structuring_element(_vp.SHAPE_RECT, int(x), int(y))


def _morph(op, mat, kernel, iterations, anchor=(-1, -1)):
    mat = as_mat(mat)
    if not isinstance(mat, (np.ndarray, DeviceMat)) or mat.dtype != np.uint8 or mat.ndim not in (2, 3):
        raise TypeError("expected a uint8 (h, w) or (h, w, c) image")
    if kernel is None or np.size(kernel) == 0:
        kp, kw, kh = None, 0, 0
    else:
        kernel = np.ascontiguousarray(np.asarray(kernel) != 0, dtype=np.uint8)
        if kernel.ndim != 2:
            raise ValueError("kernel must be 2-D")
        kh, kw = kernel.shape
        kp = _vp.ptr(kernel)
    ctx = _vp.default_context()
    if (lazy_enabled() or isinstance(mat, DeviceMat)) and mat.size and (mat.ndim == 2 or mat.shape[2] <= 4):
        # device-resident: the result stays in HBM; a mask known to be 0/255 takes the bit-plane path without a flag read-back
        src = device_image(ctx, mat, 0)
        h, w = src.shape[:2]
        cn = 1 if src.ndim == 2 else src.shape[2]
        binary = src.binary
        ax, ay, it = int(anchor[0]), int(anchor[1]), int(iterations)

        def run(out, src=src, kernel=kernel):          # (keeps the source image and the kernel array alive until it has run)
            _vp.check(_vp.lib().vp_morph_u8_dev(ctx.handle, op, src.dev_ptr, w, h, cn, kp, kw, kh, ax, ay, it, 1 if binary else 0, out.dev_ptr), ctx.handle)
        if defer_enabled() and not src.host_escaped:   # (an image whose host copy is aliased by the caller can change without notice: launch now)
            if it < 0 or (kp is not None and (ax >= kw or ay >= kh)):
                raise _vp.VpError("libvp: invalid argument: structuring element")   # what the launch would report, reported at the call
            return DeviceMat.deferred(ctx, src.shape, np.uint8, binary, (src,), run)
        out = DeviceMat(ctx, src.shape, binary=binary)
        run(out)
        return out
    src = np.ascontiguousarray(mat)
    h, w = src.shape[:2]
    cn = 1 if src.ndim == 2 else src.shape[2]
    out = np.empty_like(src)
    _vp.check(_vp.lib().vp_morph_u8(ctx.handle, op, _vp.ptr(src), w, h, cn, kp, kw, kh, int(anchor[0]), int(anchor[1]),
                                    int(iterations), _vp.ptr(out)), ctx.handle)
    return out


def erode(mat: np.ndarray, kernel: np.ndarray, iterations: int = 1) -> np.ndarray:
    """utils/transform.py:80-94 (cv2.erode)."""
    return _morph(_vp.MORPH_ERODE, mat, kernel, iterations)


def dilate(mat: np.ndarray, kernel: np.ndarray, iterations: int = 1) -> np.ndarray:
    """utils/transform.py:97-112 (cv2.dilate)."""
    return _morph(_vp.MORPH_DILATE, mat, kernel, iterations)


def morph_remove_noise(mat: np.ndarray, kernel: np.ndarray, iterations: int = 1) -> np.ndarray:
    """utils/transform.py:115-129 (cv2.morphologyEx MORPH_OPEN)."""
    return _morph(_vp.MORPH_OPEN, mat, kernel, iterations)


def morph_close_holes(mat: np.ndarray, kernel: np.ndarray, iterations: int = 1) -> np.ndarray:
    """utils/transform.py:132-146 (cv2.morphologyEx MORPH_CLOSE)."""
    return _morph(_vp.MORPH_CLOSE, mat, kernel, iterations)


def morph_borders(mat: np.ndarray, kernel: np.ndarray, iterations: int = 1) -> np.ndarray:
    """utils/transform.py:149-164 (cv2.morphologyEx MORPH_GRADIENT)."""
    return _morph(_vp.MORPH_GRADIENT, mat, kernel, iterations)


def resize(mat: np.ndarray, width: int, height: int) -> np.ndarray:
    """utils/transform.py:167-179 (cv2.resize, default bilinear interpolation) on the GPU (libvp vp_resize_u8)."""
    from vision import cv2_facade
    return cv2_facade.resize(mat, (width, height))



def simple_gaussian_blur(mat: np.ndarray, kernel_size: int, std_dev: float) -> np.ndarray:
    """utils/transform.py:3-25 (cv2.GaussianBlur with a square kernel); ValueError for an even kernel size as in the reference."""
    if kernel_size % 2 == 0:
        raise ValueError("kernel_size must be an odd integer")
    from vision import cv2_facade
    return cv2_facade.GaussianBlur(mat, (kernel_size, kernel_size), std_dev)


def median_blur(mat: np.ndarray, ksize: int) -> np.ndarray:
    """cv2.medianBlur on uint8 images of 1..4 channels, ksize odd in 1..255 (libvp vp_median_blur_u8 / vp_median_blur_dev).  Not a name
    of the reference's utils/transform.py: the despeckling step in front of a labelling or a contour pass that keeps thin structures
    (OPEN 5x5 eats them).  numpy in gives numpy out; a DeviceMat gives a DeviceMat and stays in HBM.  On a mask this library made
    (`binary`) the filter is a majority vote on the mask's bit plane, the result is a mask again and brings its own bit plane where
    rows are whole words, so range_threshold -> median_blur -> connected_components / find_contours never unpacks a bit."""
    mat = as_mat(mat)
    if not isinstance(mat, (np.ndarray, DeviceMat)) or mat.dtype != np.uint8 or mat.ndim not in (2, 3) or mat.size == 0:
        raise TypeError("expected a non-empty uint8 (h, w) or (h, w, c) image")
    cn = 1 if mat.ndim == 2 else mat.shape[2]
    if cn > 4:
        raise ValueError("at most 4 channels")
    ksize = int(ksize)
    if ksize <= 0 or ksize % 2 == 0 or ksize > 255:
        raise ValueError("ksize must be an odd integer in 1..255")
    ctx = _vp.default_context()
    h, w = mat.shape[:2]
    if isinstance(mat, DeviceMat):
        from vision.devmat import _DevBuf
        mat.refresh_device(ctx)
        src_ptr = mat.dev_ptr                            # (launches a deferred source: its bit plane comes out of that launch)
        binary = mat.binary                              # the median of 0 / 255 values is 0 or 255, whatever the channels and the window
        vote = binary and cn == 1 and 3 <= ksize <= 63   # what the bit-plane kernel serves: only then is a plane of use (the hint is ignored elsewhere)
        plane = mat.bit_plane(ctx) if (vote and mat.ndim == 2) else None
        out = DeviceMat(ctx, mat.shape, binary=binary)
        bits = _DevBuf(ctx, h * (w // 64) * 8) if (vote and mat.ndim == 2 and w % 64 == 0) else None
        made = _vp.C.c_int(0)
        _vp.check(_vp.lib().vp_median_blur_dev(ctx.handle, src_ptr, w * cn, w, h, cn, ksize, 1 if binary else 0, None if plane is None else plane.ptr,
                                               out.dev_ptr, None if bits is None else bits.ptr, _vp.C.byref(made)), ctx.handle)
        if made.value:
            out._bits = bits
        return out
    src = np.ascontiguousarray(mat)
    out = np.empty_like(src)
    _vp.check(_vp.lib().vp_median_blur_u8(ctx.handle, _vp.ptr(src), w, h, cn, ksize, _vp.ptr(out)), ctx.handle)
    return out


_DEPTH_DTYPE = {_vp.DEPTH_8U: np.uint8, _vp.DEPTH_16S: np.int16, _vp.DEPTH_32F: np.float32, _vp.DEPTH_64F: np.float64}
_BORDERS = (_vp.BORDER_CONSTANT, _vp.BORDER_REPLICATE, _vp.BORDER_REFLECT, _vp.BORDER_REFLECT_101)


def _deriv_source(mat):
    """The checked source of a derivative filter: uint8, (h, w) or (h, w, 1..4), not empty; and its channel count."""
    mat = as_mat(mat)
    if not isinstance(mat, (np.ndarray, DeviceMat)) or mat.dtype != np.uint8 or mat.ndim not in (2, 3) or mat.size == 0:
        raise TypeError("expected a non-empty uint8 (h, w) or (h, w, c) image")
    cn = 1 if mat.ndim == 2 else mat.shape[2]
    if cn > 4:
        raise ValueError("at most 4 channels")
    return mat, cn


def _deriv(mat, op, dx, dy, ksize, ddepth, border):
    """libvp vp_deriv_u8 / vp_deriv_dev: numpy in gives numpy out, a DeviceMat gives a DeviceMat of the requested dtype and stays in HBM.
    What the library refuses (orders, kernel sizes, depths, borders) comes back as ValueError before anything is launched."""
    mat, cn = _deriv_source(mat)
    dx, dy, ksize, ddepth, border = int(dx), int(dy), int(ksize), int(ddepth), int(border) & ~_vp.BORDER_ISOLATED
    depth = _vp.DEPTH_8U if ddepth == -1 else ddepth
    if depth not in _DEPTH_DTYPE:
        raise ValueError("ddepth must be -1, CV_8U, CV_16S, CV_32F or CV_64F")
    if border not in _BORDERS:
        raise ValueError("the border must be BORDER_REFLECT_101, BORDER_REPLICATE, BORDER_REFLECT or BORDER_CONSTANT")
    if op == _vp.DERIV_SOBEL and ksize == -1:
        op = _vp.DERIV_SCHARR
    if op == _vp.DERIV_SCHARR:
        if dx < 0 or dy < 0 or dx + dy != 1:
            raise ValueError("Scharr takes dx + dy == 1")
    elif op == _vp.DERIV_SOBEL:
        if not (0 <= dx <= 2 and 0 <= dy <= 2 and dx + dy > 0):
            raise ValueError("dx and dy must be in 0..2 and not both 0")
        if ksize not in (1, 3, 5, 7):
            raise ValueError("ksize must be 1, 3, 5 or 7 (or -1 for Scharr)")
        if ksize > 1 and max(dx, dy) >= ksize:
            raise ValueError("the derivative order must be below ksize")
    elif ksize not in (1, 3, 5, 7):
        raise ValueError("ksize must be 1, 3, 5 or 7")
    ctx = _vp.default_context()
    h, w = mat.shape[:2]
    dtype = _DEPTH_DTYPE[depth]
    if isinstance(mat, DeviceMat):
        mat.refresh_device(ctx)
        out = DeviceMat(ctx, mat.shape, dtype)
        _vp.check(_vp.lib().vp_deriv_dev(ctx.handle, mat.dev_ptr, w * cn, w, h, cn, op, dx, dy, ksize, depth, border, out.dev_ptr), ctx.handle)
        return out
    src = np.ascontiguousarray(mat)
    out = np.empty(src.shape, dtype)
    _vp.check(_vp.lib().vp_deriv_u8(ctx.handle, _vp.ptr(src), w, h, cn, op, dx, dy, ksize, depth, border, _vp.ptr(out)), ctx.handle)
    return out


def sobel(mat: np.ndarray, dx: int, dy: int, ksize: int = 3, ddepth: int = _vp.DEPTH_16S, border: int = _vp.BORDER_REFLECT_101) -> np.ndarray:
    """cv2.Sobel with scale 1 and delta 0 on uint8 images of 1..4 channels: the exact integer correlation with the taps of
    cv2.getDerivKernels (ksize 1, 3, 5, 7; -1 is Scharr), cast as saturate_cast does to ddepth (a libvp DEPTH_* code = cv2's CV_8U,
    CV_16S, CV_32F, CV_64F; the default here is int16, which keeps the sign).  Not a name of the reference's utils/transform.py."""
    return _deriv(mat, _vp.DERIV_SOBEL, dx, dy, ksize, ddepth, border)


def scharr(mat: np.ndarray, dx: int, dy: int, ddepth: int = _vp.DEPTH_16S, border: int = _vp.BORDER_REFLECT_101) -> np.ndarray:
    """cv2.Scharr with scale 1 and delta 0: [-1 0 1] along the differentiated axis, [3 10 3] along the other; dx + dy == 1."""
    return _deriv(mat, _vp.DERIV_SCHARR, dx, dy, 3, ddepth, border)


def laplacian(mat: np.ndarray, ksize: int = 1, ddepth: int = _vp.DEPTH_16S, border: int = _vp.BORDER_REFLECT_101) -> np.ndarray:
    """cv2.Laplacian with scale 1 and delta 0: the 3x3 kernels of ksize 1 and 3, Sobel(2, 0) + Sobel(0, 2) at ksize 5 and 7."""
    return _deriv(mat, _vp.DERIV_LAPLACIAN, 0, 0, ksize, ddepth, border)


def spatial_gradient(mat: np.ndarray, ksize: int = 3, border: int = _vp.BORDER_REFLECT_101):
    """cv2.spatialGradient: (Sobel(1, 0, 3), Sobel(0, 1, 3)) of a single-channel uint8 image, both int16, from one pass over the
    source (libvp vp_spatial_gradient_*).  ksize 3 and BORDER_REFLECT_101 or BORDER_REPLICATE only, as cv2."""
    mat, cn = _deriv_source(mat)
    if mat.ndim == 3 and cn == 1:
        mat = mat.reshaped(mat.shape[:2]) if isinstance(mat, DeviceMat) else mat[:, :, 0]
    if mat.ndim != 2:
        raise ValueError("spatial_gradient takes a single-channel image")
    ksize, border = int(ksize), int(border) & ~_vp.BORDER_ISOLATED
    if ksize != 3:
        raise ValueError("ksize must be 3")
    if border not in (_vp.BORDER_REFLECT_101, _vp.BORDER_REPLICATE):
        raise ValueError("the border must be BORDER_DEFAULT or BORDER_REPLICATE")
    ctx = _vp.default_context()
    h, w = mat.shape
    if isinstance(mat, DeviceMat):
        mat.refresh_device(ctx)
        gx, gy = DeviceMat(ctx, (h, w), np.int16), DeviceMat(ctx, (h, w), np.int16)
        _vp.check(_vp.lib().vp_spatial_gradient_dev(ctx.handle, mat.dev_ptr, w, w, h, ksize, border, gx.dev_ptr, gy.dev_ptr), ctx.handle)
        return gx, gy
    src = np.ascontiguousarray(mat)
    gx, gy = np.empty((h, w), np.int16), np.empty((h, w), np.int16)
    _vp.check(_vp.lib().vp_spatial_gradient_u8(ctx.handle, _vp.ptr(src), w, h, ksize, border, _vp.ptr(gx), _vp.ptr(gy)), ctx.handle)
    return gx, gy


def convert_scale_abs(mat: np.ndarray) -> np.ndarray:
    """cv2.convertScaleAbs with alpha 1 and beta 0: saturate_cast<uchar>(|v|) of a uint8, int16, float32 or float64 image (a float is
    rounded half to even first).  numpy in gives numpy out; a DeviceMat (a derivative that stayed in HBM) gives a uint8 DeviceMat."""
    mat = as_mat(mat)
    depth = {np.dtype(v): k for k, v in _DEPTH_DTYPE.items()}.get(np.dtype(mat.dtype)) if isinstance(mat, (np.ndarray, DeviceMat)) else None
    if depth is None or mat.ndim not in (2, 3) or mat.size == 0:
        raise TypeError("expected a non-empty uint8, int16, float32 or float64 (h, w) or (h, w, c) image")
    if mat.ndim == 3 and mat.shape[2] > 4:
        raise ValueError("at most 4 channels")
    ctx = _vp.default_context()
    if isinstance(mat, DeviceMat):
        mat.refresh_device(ctx)
        out = DeviceMat(ctx, mat.shape)
        _vp.check(_vp.lib().vp_convert_scale_abs_dev(ctx.handle, mat.dev_ptr, depth, mat.size, out.dev_ptr), ctx.handle)
        return out
    src = np.ascontiguousarray(mat)
    out = np.empty(src.shape, np.uint8)
    _vp.check(_vp.lib().vp_convert_scale_abs_u8(ctx.handle, _vp.ptr(src), depth, src.size, _vp.ptr(out)), ctx.handle)
    return out


def rotate(mat: np.ndarray, degrees: float) -> np.ndarray:
    """utils/transform.py:180-196: rotation about the image centre, positive = counterclockwise, borders replicated."""
    from vision import cv2_facade
    rot_mat = cv2_facade.getRotationMatrix2D((mat.shape[1] / 2, mat.shape[0] / 2), degrees, 1)
    return cv2_facade.warpAffine(mat, rot_mat, (mat.shape[1], mat.shape[0]), borderMode=cv2_facade.BORDER_REPLICATE)


def translate(mat: np.ndarray, x: int, y: int) -> np.ndarray:
    """utils/transform.py:199-215: shift by (x, y); uncovered pixels become 0.  The matrix goes through float32 as in the reference."""
    from vision import cv2_facade
    trans_mat = np.float32([[1, 0, x], [0, 1, y]])
    return cv2_facade.warpAffine(mat, trans_mat, (mat.shape[1], mat.shape[0]))


def decode_normal(mat: np.ndarray) -> np.ndarray:
    """utils/transform.py:218-233 (modules/normal.py:26): [0, 255] normal map back to float32 vectors in [-1, 1]; plain numpy in the
    reference as well, same operations in the same order."""
    img = np.asarray(mat).astype(np.float32)
    img = (img / 255.0) * 2.0 - 1.0
    return img
