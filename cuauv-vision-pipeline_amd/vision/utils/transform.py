"""Mirror of the reference utils/transform.py for the hot path.

Reference: utils/transform.py:27-77 (`elliptic_kernel`, `rect_kernel`), :80-112 (`erode`, `dilate`),
:115-164 (`morph_remove_noise`, `morph_close_holes`, `morph_borders`).  Kernels: libvp vp_morph_u8
(bit-plane LDS stencils for 0/255 masks with rect kernels, generic kernel otherwise).
"""
from typing import Optional

import numpy as np

from vision import _vp
from vision.devmat import DeviceMat, _DevBuf, defer_enabled, finish_uploads, lazy_enabled
from vision.utils.helpers import as_cv2_error, as_mat, device_image, error, image_source, packed_source, run_operator


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
    return _resize(mat, (width, height))


def _plain_source(name, src, words):
    """The source of the operators that came with cv2's names and refuse in cv2's way (cv2.error, one sentence for a wrong dtype, a
    wrong shape and no pixels; more than 4 channels is refused with the operator's sizes)."""
    return as_cv2_error(name, image_source, packed_source(src)[0], said=(words, words, None))


def _resize(src, dsize, fx=None, fy=None, interpolation=_vp.INTER_LINEAR):
    """cv2.resize without dst (libvp vp_resize_u8 / vp_resize_u8_scaled / vp_resize_dev); dsize None or (0, 0) takes the size from fx / fy."""
    if interpolation != _vp.INTER_LINEAR:
        raise error("resize: only INTER_LINEAR is on the accelerated path")
    src, _ = packed_source(src)
    scaled = dsize is None or tuple(dsize) == (0, 0)
    if scaled:
        if not fx or not fy or not (fx > 0 and fy > 0):
            raise error("resize: dsize or both fx and fy (positive) are needed")
        fx, fy = float(fx), float(fy)                # cv2 keeps them as the inverse scales: the tables use 1 / fx, not size / dsize
        dsize = (int(round(src.shape[1] * fx)), int(round(src.shape[0] * fy)))   # cv2: saturate_cast<int>(cols * fx): round half to even
    # (cv2 ignores fx / fy when dsize is given)
    src, cn = _plain_source("resize", src, "expected a non-empty uint8 image")
    dw, dh = int(dsize[0]), int(dsize[1])
    if dw <= 0 or dh <= 0 or cn > 4:
        raise error("resize: bad size")
    h, w = src.shape[:2]
    lib = _vp.lib()
    sx, sy = (fx, fy) if scaled else (0.0, 0.0)      # the device entry takes scales <= 0 as dsize / ssize

    def host_call(ctx, s, d):
        if scaled:
            return lib.vp_resize_u8_scaled(ctx.handle, s, w, h, cn, dw, dh, fx, fy, d)
        return lib.vp_resize_u8(ctx.handle, s, w, h, cn, dw, dh, d)
    try:
        return run_operator(src, (dh, dw) + tuple(src.shape[2:]), np.uint8, host_call,
                            lambda ctx, s, d: lib.vp_resize_dev(ctx.handle, s, w * cn, w, h, cn, dw, dh, sx, sy, d))
    except _vp.VpError as e:                         # scale 2 with a partial edge cell: not reproduced
        raise error(f"resize: {e}") from e


def _gaussian_blur(src, ksize, sigma_x, sigma_y=0, border=None):
    """cv2.GaussianBlur without dst: OpenCV's bit-exact fixed-point path (libvp vp_gaussian_blur_u8 / vp_gaussian_blur_dev)."""
    if border not in (None, _vp.BORDER_REFLECT_101):
        raise error("GaussianBlur: only BORDER_DEFAULT (reflect 101) is on the accelerated path")
    src, cn = _plain_source("GaussianBlur", src, "only non-empty uint8 images are on the accelerated path")
    kw, kh = int(ksize[0]), int(ksize[1])
    if kw <= 0 or kh <= 0 or kw % 2 == 0 or kh % 2 == 0 or kw > 511 or kh > 511 or cn > 4:
        raise error("GaussianBlur: kernel sizes must be odd, 1..511")
    h, w = src.shape[:2]
    sx, sy = float(sigma_x), float(sigma_y)
    lib = _vp.lib()
    return run_operator(src, src.shape, np.uint8,
                        lambda ctx, s, d: lib.vp_gaussian_blur_u8(ctx.handle, s, w, h, cn, kw, kh, sx, sy, d),
                        lambda ctx, s, d: lib.vp_gaussian_blur_dev(ctx.handle, s, w * cn, w, h, cn, kw, kh, sx, sy, d))


def simple_gaussian_blur(mat: np.ndarray, kernel_size: int, std_dev: float) -> np.ndarray:
    """utils/transform.py:3-25 (cv2.GaussianBlur with a square kernel); ValueError for an even kernel size as in the reference."""
    if kernel_size % 2 == 0:
        raise ValueError("kernel_size must be an odd integer")
    return _gaussian_blur(mat, (kernel_size, kernel_size), std_dev)


def median_blur(mat: np.ndarray, ksize: int) -> np.ndarray:
    """cv2.medianBlur on uint8 images of 1..4 channels, ksize odd in 1..255 (libvp vp_median_blur_u8 / vp_median_blur_dev).  Not a name
    of the reference's utils/transform.py: the despeckling step in front of a labelling or a contour pass that keeps thin structures
    (OPEN 5x5 eats them).  numpy in gives numpy out; a DeviceMat gives a DeviceMat and stays in HBM.  On a mask this library made
    (`binary`) the filter is a majority vote on the mask's bit plane, the result is a mask again and brings its own bit plane where
    rows are whole words, so range_threshold -> median_blur -> connected_components / find_contours never unpacks a bit."""
    mat, cn = image_source(mat)
    ksize = int(ksize)
    if ksize <= 0 or ksize % 2 == 0 or ksize > 255:
        raise ValueError("ksize must be an odd integer in 1..255")
    h, w = mat.shape[:2]
    lib = _vp.lib()
    binary = isinstance(mat, DeviceMat) and mat.binary   # the median of 0 / 255 values is 0 or 255, whatever the channels and the window
    vote = binary and mat.ndim == 2 and 3 <= ksize <= 63   # what the bit-plane kernel serves: only then is a plane of use (the hint is ignored elsewhere)
    made, bits = _vp.C.c_int(0), None

    def dev_call(ctx, s, d):                             # (the source has been launched by now: its bit plane comes out of that launch)
        nonlocal bits
        plane = mat.bit_plane(ctx) if vote else None
        bits = _DevBuf(ctx, h * (w // 64) * 8) if (vote and w % 64 == 0) else None
        return lib.vp_median_blur_dev(ctx.handle, s, w * cn, w, h, cn, ksize, 1 if binary else 0, None if plane is None else plane.ptr, d,
                                      None if bits is None else bits.ptr, _vp.C.byref(made))
    out = run_operator(mat, mat.shape, np.uint8, lambda ctx, s, d: lib.vp_median_blur_u8(ctx.handle, s, w, h, cn, ksize, d), dev_call, binary)
    if made.value:
        out._bits = bits
    return out


_DEPTH_DTYPE = {_vp.DEPTH_8U: np.uint8, _vp.DEPTH_16S: np.int16, _vp.DEPTH_32F: np.float32, _vp.DEPTH_64F: np.float64}
_DTYPE_DEPTH = {np.dtype(v): k for k, v in _DEPTH_DTYPE.items()}
_BORDERS = (_vp.BORDER_CONSTANT, _vp.BORDER_REPLICATE, _vp.BORDER_REFLECT, _vp.BORDER_REFLECT_101)


def _deriv(mat, op, dx, dy, ksize, ddepth, border):
    """libvp vp_deriv_u8 / vp_deriv_dev: numpy in gives numpy out, a DeviceMat gives a DeviceMat of the requested dtype and stays in HBM.
    What the library refuses (orders, kernel sizes, depths, borders) comes back as ValueError before anything is launched."""
    mat, cn = image_source(mat)
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
    h, w = mat.shape[:2]
    lib = _vp.lib()
    return run_operator(mat, mat.shape, _DEPTH_DTYPE[depth],
                        lambda ctx, s, d: lib.vp_deriv_u8(ctx.handle, s, w, h, cn, op, dx, dy, ksize, depth, border, d),
                        lambda ctx, s, d: lib.vp_deriv_dev(ctx.handle, s, w * cn, w, h, cn, op, dx, dy, ksize, depth, border, d))


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
    mat, _ = image_source(mat, single="spatial_gradient takes a single-channel image")
    ksize, border = int(ksize), int(border) & ~_vp.BORDER_ISOLATED
    if ksize != 3:
        raise ValueError("ksize must be 3")
    if border not in (_vp.BORDER_REFLECT_101, _vp.BORDER_REPLICATE):
        raise ValueError("the border must be BORDER_DEFAULT or BORDER_REPLICATE")
    h, w = mat.shape
    lib = _vp.lib()
    return run_operator(mat, (h, w), np.int16,
                        lambda ctx, s, gx, gy: lib.vp_spatial_gradient_u8(ctx.handle, s, w, h, ksize, border, gx, gy),
                        lambda ctx, s, gx, gy: lib.vp_spatial_gradient_dev(ctx.handle, s, w, w, h, ksize, border, gx, gy), pair=True)


def convert_scale_abs(mat: np.ndarray) -> np.ndarray:
    """cv2.convertScaleAbs with alpha 1 and beta 0: saturate_cast<uchar>(|v|) of a uint8, int16, float32 or float64 image (a float is
    rounded half to even first).  numpy in gives numpy out; a DeviceMat (a derivative that stayed in HBM) gives a uint8 DeviceMat."""
    mat, _ = image_source(mat, dtypes=_DTYPE_DEPTH)
    depth = _DTYPE_DEPTH[mat.dtype]
    n = mat.size
    lib = _vp.lib()
    return run_operator(mat, mat.shape, np.uint8,
                        lambda ctx, s, d: lib.vp_convert_scale_abs_u8(ctx.handle, s, depth, n, d),
                        lambda ctx, s, d: lib.vp_convert_scale_abs_dev(ctx.handle, s, depth, n, d))


_BOX_DTYPE = {_vp.DEPTH_8U: np.uint8, _vp.DEPTH_16S: np.int16, _vp.DEPTH_32S: np.int32, _vp.DEPTH_32F: np.float32, _vp.DEPTH_64F: np.float64}
BOX_MAX_SIDE = 255


def box_filter(mat: np.ndarray, kx: int, ky: Optional[int] = None, ddepth: int = -1, normalize: bool = True, border: int = _vp.BORDER_REFLECT_101):
    """cv2.boxFilter on uint8 images of 1..4 channels (libvp vp_box_filter_u8 / vp_box_filter_dev): the sum over the ky x kx window
    anchored at (kx // 2, ky // 2).  Unnormalised it is cast to ddepth (-1 / CV_8U and CV_16S saturate; CV_32S, CV_32F, CV_64F); normalised
    (uint8 only) it is sum / area rounded as OpenCV rounds, for the areas on which OpenCV's own roundings agree - the others raise
    ValueError before anything is launched.  numpy in gives numpy out; a DeviceMat gives a DeviceMat of the result's dtype, without
    the source's mask flag and bit plane: the result is no mask."""
    mat, cn = image_source(mat)
    kx = int(kx)
    ky = kx if ky is None else int(ky)
    ddepth, border, normalize = int(ddepth), int(border) & ~_vp.BORDER_ISOLATED, bool(normalize)
    depth = _vp.DEPTH_8U if ddepth == -1 else ddepth
    if not (1 <= kx <= BOX_MAX_SIDE and 1 <= ky <= BOX_MAX_SIDE):
        raise ValueError("the window sides must be in 1..255")
    if depth not in _BOX_DTYPE:
        raise ValueError("ddepth must be -1, CV_8U, CV_16S, CV_32S, CV_32F or CV_64F")
    if border not in _BORDERS:
        raise ValueError("the border must be BORDER_REFLECT_101, BORDER_REPLICATE, BORDER_REFLECT or BORDER_CONSTANT")
    if normalize:
        if depth != _vp.DEPTH_8U:
            raise ValueError("a normalised box filter gives CV_8U only: OpenCV's float scaling of the other depths is not restated")
        if _vp.lib().vp_box_area_exact(kx * ky) != 1:
            raise ValueError("OpenCV's roundings of sum / area disagree for a window of %d pixels: it cannot be restated" % (kx * ky))
    elif depth == _vp.DEPTH_32F and 255 * kx * ky >= 1 << 24:
        raise ValueError("the window's sum may not be exact in float32: ask for CV_32S or CV_64F")
    h, w = mat.shape[:2]
    lib = _vp.lib()
    return run_operator(mat, mat.shape, _BOX_DTYPE[depth],
                        lambda ctx, s, d: lib.vp_box_filter_u8(ctx.handle, s, w, h, cn, kx, ky, int(normalize), depth, border, d),
                        lambda ctx, s, d: lib.vp_box_filter_dev(ctx.handle, s, w * cn, w, h, cn, kx, ky, int(normalize), depth, border, d))


def box_blur(mat: np.ndarray, kx: int, ky: Optional[int] = None) -> np.ndarray:
    """cv2.blur(mat, (kx, ky)): the normalised box filter with the default border."""
    return box_filter(mat, kx, ky)


def _pyr(mat, down, border):
    mat, cn = image_source(mat)
    border = int(border) & ~_vp.BORDER_ISOLATED
    if down and border not in (_vp.BORDER_REFLECT_101, _vp.BORDER_REPLICATE, _vp.BORDER_REFLECT):
        raise ValueError("pyrDown takes BORDER_REFLECT_101, BORDER_REPLICATE or BORDER_REFLECT")
    if not down and border != _vp.BORDER_REFLECT_101:
        raise ValueError("pyrUp takes BORDER_DEFAULT only")
    h, w = mat.shape[:2]
    if h > 32767:
        raise ValueError("at most 32767 rows")
    oh, ow = ((h + 1) // 2, (w + 1) // 2) if down else (2 * h, 2 * w)
    shape = (oh, ow) + tuple(mat.shape[2:])
    L = _vp.lib()
    if down:
        return run_operator(mat, shape, np.uint8, lambda ctx, s, d: L.vp_pyr_down_u8(ctx.handle, s, w, h, cn, border, d),
                            lambda ctx, s, d: L.vp_pyr_down_dev(ctx.handle, s, w * cn, w, h, cn, border, d))
    return run_operator(mat, shape, np.uint8, lambda ctx, s, d: L.vp_pyr_up_u8(ctx.handle, s, w, h, cn, d),
                        lambda ctx, s, d: L.vp_pyr_up_dev(ctx.handle, s, w * cn, w, h, cn, d))


def pyr_down(mat: np.ndarray, border: int = _vp.BORDER_REFLECT_101) -> np.ndarray:
    """cv2.pyrDown on uint8 images of 1..4 channels: ((w + 1) // 2, (h + 1) // 2), the 5 x 5 binomial kernel at every second pixel
    (libvp vp_pyr_down_*).  numpy in gives numpy out; a DeviceMat gives a DeviceMat and stays in HBM."""
    return _pyr(mat, True, border)


def pyr_up(mat: np.ndarray, border: int = _vp.BORDER_REFLECT_101) -> np.ndarray:
    """cv2.pyrUp on uint8 images of 1..4 channels: (2w, 2h), OpenCV's polyphase form of the same kernel (libvp vp_pyr_up_*)."""
    return _pyr(mat, False, border)


def build_pyramid(mat: np.ndarray, levels: int) -> list:
    """cv2.buildPyramid: [mat, pyr_down(mat), ...], levels + 1 images.  The levels of a DeviceMat are DeviceMats made from each other
    in HBM; a numpy source is uploaded once, the levels are made on the device and each is brought back."""
    levels = int(levels)
    if levels < 0:
        raise ValueError("levels must not be negative")
    src, _ = image_source(mat)
    if isinstance(src, DeviceMat):
        out = [src]
        for _ in range(levels):
            out.append(pyr_down(out[-1]))
        return out
    ctx = _vp.default_context()
    dev = [device_image(ctx, np.ascontiguousarray(src), 0)]
    for _ in range(levels):
        dev.append(pyr_down(dev[-1]))
    return [np.ascontiguousarray(src)] + [d.host_copy() for d in dev[1:]]


def integral(mat: np.ndarray) -> np.ndarray:
    """cv2.integral on uint8 images of 1..4 channels: the (h + 1, w + 1[, cn]) int32 image of sums above and left of every pixel
    (libvp vp_integral_*); 255 * w * h must fit int32.  numpy in gives numpy out; a DeviceMat gives an int32 DeviceMat."""
    mat, cn = image_source(mat)
    h, w = mat.shape[:2]
    if 255 * w * h > 2 ** 31 - 1:
        raise ValueError("255 * w * h does not fit the int32 sums")
    shape = (h + 1, w + 1) + tuple(mat.shape[2:])
    lib = _vp.lib()
    return run_operator(mat, shape, np.int32, lambda ctx, s, d: lib.vp_integral_u8(ctx.handle, s, w, h, cn, d),
                        lambda ctx, s, d: lib.vp_integral_dev(ctx.handle, s, w * cn, w, h, cn, d))


def _border_bytes(value):
    """cv2's borderValue (a Scalar: missing entries are 0) as four saturated bytes"""
    bv = np.zeros(4, np.uint8)
    vals = np.atleast_1d(np.asarray(value, dtype=np.float64)).ravel()[:4]
    bv[:len(vals)] = np.clip(np.rint(vals), 0, 255).astype(np.uint8)
    return bv


def _gather_checks(mat, border):
    mat, cn = image_source(mat, max_side=32767)
    if int(border) not in (_vp.BORDER_CONSTANT, _vp.BORDER_REPLICATE):
        raise ValueError("only BORDER_CONSTANT and BORDER_REPLICATE are on the accelerated path")
    return mat, cn


def _classify_maps(map1, map2):
    """The map forms of cv2.remap: ("planar", x, y), ("interleaved", xy, None) - float32 - or ("fixed", xy int16, fractions uint16 or
    None); and the maps' (height, width).  An empty map2 counts as none."""
    a = as_mat(map1)
    b = None if map2 is None else as_mat(map2)
    if b is not None and b.size == 0:
        b = None
    ok = lambda m: isinstance(m, (np.ndarray, DeviceMat)) and m.size > 0
    if not ok(a) or (b is not None and not ok(b)):
        raise TypeError("the maps must be non-empty arrays")
    if a.dtype == np.float32 and a.ndim == 2 and b is not None and b.dtype == np.float32 and tuple(b.shape) == tuple(a.shape):
        return "planar", a, b, tuple(a.shape)
    if a.dtype == np.float32 and a.ndim == 3 and a.shape[2] == 2 and b is None:
        return "interleaved", a, None, tuple(a.shape[:2])
    if a.dtype == np.int16 and a.ndim == 3 and a.shape[2] == 2:
        if b is None:
            return "fixed", a, None, tuple(a.shape[:2])
        if b.dtype in (np.uint16, np.int16) and tuple(b.shape) in (tuple(a.shape[:2]), tuple(a.shape[:2]) + (1,)):
            return "fixed", a, b, tuple(a.shape[:2])
    raise TypeError("the maps must be two float32 planes, one float32 (h, w, 2) plane, or an int16 (h, w, 2) plane with an optional uint16 (h, w) plane")


def _map_on_device(ctx, m, pending):
    if isinstance(m, DeviceMat):
        m.refresh_device(ctx)
        return m
    return DeviceMat.from_host(ctx, m, pending=pending)


def _remap(mat, map1, map2, nearest, border=_vp.BORDER_CONSTANT, border_value=0):
    """libvp vp_remap_u8 / vp_remap_f32_dev / vp_remap_fixed_dev.  A DeviceMat source gives a DeviceMat and stays in HBM (maps that are
    numpy arrays are uploaded); a numpy source gives numpy.  Nothing is launched for arguments outside the path: they raise."""
    mat, cn = _gather_checks(mat, border)
    kind, a, b, (mh, mw) = _classify_maps(map1, map2)
    nearest = bool(nearest)
    if kind == "fixed" and nearest and b is not None:
        raise ValueError("nearest interpolation takes the int16 x,y plane alone (cv2 rounds by the fraction plane there: DESIGN.md section 7)")
    if kind == "fixed" and not nearest and b is None:
        raise ValueError("an int16 x,y plane alone is a nearest-neighbour map: pass INTER_NEAREST, or the fraction plane")
    if mh > 65535 or mw > (1 << 24) or mh * mw >= (1 << 31):
        raise ValueError("the maps are larger than 65535 rows, 2^24 columns or 2^31 entries")
    interp = _vp.INTER_NEAREST if nearest else _vp.INTER_LINEAR
    bv = _border_bytes(border_value)
    ctx = _vp.default_context()
    lib = _vp.lib()
    h, w = mat.shape[:2]
    on_dev = isinstance(mat, DeviceMat)
    on_host = not on_dev and kind != "fixed" and isinstance(a, np.ndarray) and (b is None or isinstance(b, np.ndarray))
    entry = lib.vp_remap_fixed_dev if kind == "fixed" else lib.vp_remap_f32_dev
    up = []
    try:
        if on_host:                                      # the host entry reads the float maps where they are
            src, a, b = mat, np.ascontiguousarray(a), None if b is None else np.ascontiguousarray(b)
        else:                                            # whatever is not on the device yet is uploaded, the source included
            src = mat if on_dev else DeviceMat.from_host(ctx, mat, pending=up)
            a, b = _map_on_device(ctx, a, up), None if b is None else _map_on_device(ctx, b, up)
        out = run_operator(src, (mh, mw) + tuple(mat.shape[2:]), np.uint8,
                           lambda ctx, s, d: lib.vp_remap_u8(ctx.handle, s, w, h, cn, _vp.ptr(a), _vp.ptr(b), mw, mh, interp, int(border), _vp.ptr(bv), d),
                           lambda ctx, s, d: entry(ctx.handle, s, w * cn, w, h, cn, a.dev_ptr, None if b is None else b.dev_ptr, mw, mh, interp,
                                                   int(border), _vp.ptr(bv), d))
    finally:
        finish_uploads(ctx, up)
    return out if on_dev or on_host else out.host_copy()


def remap(mat: np.ndarray, map_x, map_y=None, nearest: bool = False, border: int = _vp.BORDER_CONSTANT, border_value=0) -> np.ndarray:
    """cv2.remap on uint8 images of 1..4 channels with bilinear (default) or nearest-neighbour interpolation, OpenCV's classical
    fixed-point path byte for byte.  Maps, numpy or DeviceMat: two float32 planes; one float32 (h, w, 2)
    plane; the fixed form of cv2.convertMaps (int16 (h, w, 2) + uint16 (h, w)); or an int16 (h, w, 2) plane alone with nearest=True.
    The result has the maps' size.  Maps that stay the same from frame to frame belong in a RemapTable.  Not a name of the
    reference's utils/transform.py."""
    return _remap(mat, map_x, map_y, nearest, border, border_value)


class RemapTable:
    """Float maps turned once into the fixed form (int16 coordinates + 5 + 5 bit fractions, libvp vp_convert_maps_dev) and kept in
    HBM: 6 bytes per destination pixel (4 for nearest) instead of 8.  `apply` is one launch (vp_remap_fixed_dev) and gives the bytes
    `remap` gives from the float maps."""

    def __init__(self, map_x, map_y=None, nearest: bool = False):
        kind, a, b, (mh, mw) = _classify_maps(map_x, map_y)
        if kind == "fixed":
            raise TypeError("a RemapTable is built from float32 maps")
        if mh > 65535 or mw > (1 << 24):
            raise ValueError("the maps are larger than 65535 rows or 2^24 columns")
        ctx = _vp.default_context()
        self.nearest = bool(nearest)
        self.shape = (mh, mw)
        up = []
        try:
            da = _map_on_device(ctx, a, up)
            db = None if b is None else _map_on_device(ctx, b, up)
            self.xy = DeviceMat(ctx, (mh, mw, 2), np.int16)
            self.frac = None if self.nearest else DeviceMat(ctx, (mh, mw), np.uint16)
            _vp.check(_vp.lib().vp_convert_maps_dev(ctx.handle, da.dev_ptr, None if db is None else db.dev_ptr, mw, mh, int(self.nearest), self.xy.dev_ptr,
                                                    None if self.frac is None else self.frac.dev_ptr), ctx.handle)
        finally:
            finish_uploads(ctx, up)

    def apply(self, mat, border: int = _vp.BORDER_CONSTANT, border_value=0):
        """The remapped image: a DeviceMat for a DeviceMat (one launch, nothing copied), numpy for numpy."""
        return _remap(mat, self.xy, self.frac, self.nearest, border, border_value)


def undistorter(camera_matrix, dist_coeffs, size, new_camera_matrix=None) -> RemapTable:
    """The lens-undistortion table of a calibrated camera, built once: cv2.initUndistortRectifyMap (no rectification; the new camera
    matrix defaults to the camera matrix) into a RemapTable.  size = (width, height) of the undistorted image.  A module calls
    `table.apply(frame)` per frame."""
    k = camera_matrix if new_camera_matrix is None else new_camera_matrix
    u, v = _undistort_coords("initUndistortRectifyMap", camera_matrix, dist_coeffs, None, k, size)
    return RemapTable(u.astype(np.float32), v.astype(np.float32))


def _camera(name, cameraMatrix, distCoeffs):
    """(fx, fy, cx, cy), the 8 rational-model coefficients k1 k2 p1 p2 k3 k4 k5 k6 (missing ones 0), in float64"""
    A = np.asarray(cameraMatrix, dtype=np.float64)
    if A.shape != (3, 3) or not np.isfinite(A).all():
        raise error(f"{name}: the camera matrix must be a finite 3x3 matrix")
    d = np.zeros(0) if distCoeffs is None else np.asarray(distCoeffs, dtype=np.float64).ravel()
    if d.size not in (0, 4, 5, 8, 12, 14) or not np.isfinite(d).all():
        raise error(f"{name}: 4, 5, 8, 12 or 14 finite distortion coefficients")
    if d.size > 8 and np.any(d[8:] != 0):
        raise error(f"{name}: the thin-prism (s1..s4) and tilt (tauX, tauY) coefficients are outside the path (DESIGN.md section 7)")
    k = np.zeros(8)
    k[:min(d.size, 8)] = d[:8]
    return A, k


def _undistort_coords(name, cameraMatrix, distCoeffs, R, newCameraMatrix, size):
    """source coordinates (u, v), float64 (h, w) each, of every pixel of the undistorted image: the model of
    cv2.initUndistortRectifyMap evaluated per pixel (cv2 accumulates the row increments instead: not bit-exact)"""
    A, k = _camera(name, cameraMatrix, distCoeffs)
    w, h = int(size[0]), int(size[1])
    if w <= 0 or h <= 0:
        raise error(f"{name}: the size must be positive")
    Ar = A if newCameraMatrix is None else np.asarray(newCameraMatrix, dtype=np.float64)
    if Ar.shape == (3, 4):
        Ar = Ar[:, :3]
    Rm = np.eye(3) if R is None else np.asarray(R, dtype=np.float64)
    if Ar.shape != (3, 3) or Rm.shape != (3, 3) or not np.isfinite(Ar).all() or not np.isfinite(Rm).all():
        raise error(f"{name}: R and the new camera matrix must be finite 3x3 matrices")
    try:
        ir = np.linalg.inv(Ar @ Rm)
    except np.linalg.LinAlgError:
        raise error(f"{name}: newCameraMatrix * R is singular") from None
    j, i = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    X = ir[0, 0] * j + ir[0, 1] * i + ir[0, 2]
    Y = ir[1, 0] * j + ir[1, 1] * i + ir[1, 2]
    W = ir[2, 0] * j + ir[2, 1] * i + ir[2, 2]
    x, y = X / W, Y / W
    k1, k2, p1, p2, k3, k4, k5, k6 = k
    x2, y2 = x * x, y * y
    r2, xy2 = x2 + y2, 2 * x * y
    kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
    xd = x * kr + p1 * xy2 + p2 * (r2 + 2 * x2)
    yd = y * kr + p1 * (r2 + 2 * y2) + p2 * xy2
    return A[0, 0] * xd + A[0, 2], A[1, 1] * yd + A[1, 2]


def _fixed_from_double(u, v):
    """CV_16SC2 maps from double coordinates: iu = saturate_cast<int>(u * 32), integer part iu >> 5, fraction index from iu & 31.
    The integer part is saturated to int16 here; cv2 casts it to short without saturating, so the two differ beyond +-32768."""
    iu = np.clip(np.rint(u * 32), -2147483648, 2147483647).astype(np.int64)
    iv = np.clip(np.rint(v * 32), -2147483648, 2147483647).astype(np.int64)
    xy = np.stack([np.clip(iu >> 5, -32768, 32767), np.clip(iv >> 5, -32768, 32767)], axis=-1).astype(np.int16)
    return np.ascontiguousarray(xy), ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)


def _warp_perspective(mat, M, dw, dh, inverse_map=False, nearest=False, border=_vp.BORDER_CONSTANT, border_value=0):
    """libvp vp_warp_perspective_u8 / vp_warp_perspective_dev"""
    mat, cn = _gather_checks(mat, border)
    m = np.ascontiguousarray(np.asarray(M, dtype=np.float64))
    dw, dh = int(dw), int(dh)
    if m.shape != (3, 3) or not np.isfinite(m).all():
        raise ValueError("M must be a finite 3x3 matrix")
    if dw <= 0 or dh <= 0 or dh > 65535 or dw > (1 << 24) or dw * dh >= (1 << 31):
        raise ValueError("the size must be positive, at most 65535 rows, 2^24 columns and 2^31 pixels")
    flags = (_vp.WARP_INVERSE_MAP if inverse_map else 0) | (_vp.INTER_NEAREST if nearest else _vp.INTER_LINEAR)
    bv = _border_bytes(border_value)
    h, w = mat.shape[:2]
    lib = _vp.lib()
    return run_operator(mat, (dh, dw) + tuple(mat.shape[2:]), np.uint8,
                        lambda ctx, s, d: lib.vp_warp_perspective_u8(ctx.handle, s, w, h, cn, _vp.ptr(m), flags, int(border), _vp.ptr(bv), d, dw, dh),
                        lambda ctx, s, d: lib.vp_warp_perspective_dev(ctx.handle, s, w * cn, w, h, cn, _vp.ptr(m), flags, int(border), _vp.ptr(bv), d, dw, dh))


def warp_perspective(mat: np.ndarray, M, width: int, height: int) -> np.ndarray:
    """cv2.warpPerspective(mat, M, (width, height)): bilinear, uncovered pixels 0, M (3x3) maps source to destination; OpenCV's
    classical fixed-point path byte for byte.  Not a name of the reference's utils/transform.py."""
    return _warp_perspective(mat, M, width, height)


def _rotation_matrix_2d(center, angle, scale):
    """imgproc/src/imgwarp.cpp getRotationMatrix2D: 2x3 float64 (modules/preprocessor.py:131-133)."""
    ang = angle * np.pi / 180.0
    a, b = scale * np.cos(ang), scale * np.sin(ang)
    cx, cy = float(np.float32(center[0])), float(np.float32(center[1]))   # the centre is a Point2f
    return np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]], np.float64)


def _warp_affine(src, M, dsize, flags=_vp.INTER_LINEAR, border=_vp.BORDER_CONSTANT, border_value=0):
    """cv2.warpAffine without dst: OpenCV's classical fixed-point path (libvp vp_warp_affine_u8 / vp_warp_affine_dev)."""
    if flags is None:
        flags = _vp.INTER_LINEAR
    if (flags & ~_vp.WARP_INVERSE_MAP) != _vp.INTER_LINEAR:
        raise error("warpAffine: only INTER_LINEAR is on the accelerated path")
    if border not in (_vp.BORDER_CONSTANT, _vp.BORDER_REPLICATE):
        raise error("warpAffine: only BORDER_CONSTANT and BORDER_REPLICATE are on the accelerated path")
    src, cn = _plain_source("warpAffine", src, "expected a non-empty uint8 image")
    m = np.ascontiguousarray(np.asarray(M, dtype=np.float64))
    dw, dh = int(dsize[0]), int(dsize[1])
    if m.shape != (2, 3) or dw <= 0 or dh <= 0 or cn > 4:
        raise error("warpAffine: M must be 2x3 and the size positive")
    bv = _border_bytes(border_value)
    h, w = src.shape[:2]
    inverse, border = int(flags & _vp.WARP_INVERSE_MAP), int(border)
    lib = _vp.lib()
    return run_operator(src, (dh, dw) + tuple(src.shape[2:]), np.uint8,
                        lambda ctx, s, d: lib.vp_warp_affine_u8(ctx.handle, s, w, h, cn, _vp.ptr(m), inverse, border, _vp.ptr(bv), d, dw, dh),
                        lambda ctx, s, d: lib.vp_warp_affine_dev(ctx.handle, s, w * cn, w, h, cn, _vp.ptr(m), inverse, border, _vp.ptr(bv), d, dw, dh))


def rotate(mat: np.ndarray, degrees: float) -> np.ndarray:
    """utils/transform.py:180-196: rotation about the image centre, positive = counterclockwise, borders replicated."""
    rot_mat = _rotation_matrix_2d((mat.shape[1] / 2, mat.shape[0] / 2), degrees, 1)
    return _warp_affine(mat, rot_mat, (mat.shape[1], mat.shape[0]), border=_vp.BORDER_REPLICATE)


def translate(mat: np.ndarray, x: int, y: int) -> np.ndarray:
    """utils/transform.py:199-215: shift by (x, y); uncovered pixels become 0.  The matrix goes through float32 as in the reference."""
    trans_mat = np.float32([[1, 0, x], [0, 1, y]])
    return _warp_affine(mat, trans_mat, (mat.shape[1], mat.shape[0]))


def decode_normal(mat: np.ndarray) -> np.ndarray:
    """utils/transform.py:218-233 (modules/normal.py:26): [0, 255] normal map back to float32 vectors in [-1, 1]; plain numpy in the
    reference as well, same operations in the same order."""
    img = np.asarray(mat).astype(np.float32)
    img = (img / 255.0) * 2.0 - 1.0
    return img
