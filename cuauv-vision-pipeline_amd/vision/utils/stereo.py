"""Stereo block matching on the GPU: what the reference's forward camera got from its vendor SDK as the `depth` plane
(capture_sources/zed_sync.py:90-149), made here from the rectified left and right images (libvp vp_stereo.hip).

`disparity` follows the design of cv2.StereoBM - capped horizontal Sobel prefilter, sums of absolute differences over a square window,
texture and uniqueness tests, parabola subpixel - as tests/stereo_restate.py states it, byte for byte; it has not met a real OpenCV.
The pair must be rectified (vision.utils.transform.undistorter / RemapTable apply a calibration's maps): a point of `left` at column x
lies on the same row of `right` at column x - D.

After the matcher (libvp vp_speckle.hip): `filter_speckles` removes the small islands of wrong answers by the rule
of cv2.filterSpeckles, as tests/speckle_restate.py states it, byte for byte (it has not met a real OpenCV either); `normals_from_depth`
makes the reference's fourth plane, `normal` (zed_sync.py:114,132-137), by this library's own definition, bit for bit as
tests/normals_restate.py states it; `stereo_planes` chains all four steps in HBM.

`disparity_sgm` is the second matcher (libvp vp_sgm.hip): semi-global matching in the shape of cv2.StereoSGBM
with a left-right check, as tests/sgm_restate.py states it, byte for byte; it does not claim OpenCV's bits.  It answers the flat
surfaces the block matcher's texture test leaves empty.  `stereo_depth_sgm` and `stereo_planes_sgm` are the two chains on top of it.
"""
import ctypes as C

import numpy as np

from vision import _vp
from vision.devmat import DeviceMat
from vision.utils.helpers import device_image, image_source

MAX_SIDE = 4096
_RANGES = (("num_disparities", 16, 256), ("block_size", 5, 21), ("min_disparity", -128, 128), ("pre_filter_cap", 1, 63), ("texture_threshold", 0, 2 ** 31 - 1),
           ("uniqueness_ratio", 0, 100))


def _matcher(num_disparities=64, block_size=15, min_disparity=0, pre_filter_cap=31, texture_threshold=10, uniqueness_ratio=15):
    """the six checked parameters, in the order of the C entries; everything libvp refuses is refused here, before a device is needed"""
    given = (num_disparities, block_size, min_disparity, pre_filter_cap, texture_threshold, uniqueness_ratio)
    out = []
    for (name, lo, hi), v in zip(_RANGES, given):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{name} must be an integer")
        if not lo <= v <= hi:
            raise ValueError(f"{name} must lie in {lo}..{hi}")
        out.append(int(v))
    if out[0] % 16:
        raise ValueError("num_disparities must be a multiple of 16")
    if out[1] % 2 == 0:
        raise ValueError("block_size must be odd")
    return tuple(out)


def _grey(mat, which):
    mat, cn = image_source(mat, max_side=MAX_SIDE)
    if cn == 3:
        from vision.utils.color import bgr_to_gray
        mat = bgr_to_gray(mat)[0]
    elif cn != 1:
        raise ValueError(f"the {which} image must have one channel, or three (BGR)")
    if mat.ndim == 3:
        mat = mat.reshaped(mat.shape[:2]) if isinstance(mat, DeviceMat) else mat[:, :, 0]
    return mat


def _pair(left, right):
    left, right = _grey(left, "left"), _grey(right, "right")
    if tuple(left.shape) != tuple(right.shape):
        raise ValueError("the left and right images must have one size")
    return left, right


def invalid_disparity(min_disparity: int = 0) -> int:
    """the int16 value of a pixel without an answer: (min_disparity - 1) * 16"""
    return (int(min_disparity) - 1) * 16


def valid_rect(w: int, h: int, num_disparities: int = 64, block_size: int = 15, min_disparity: int = 0):
    """(x, y, w, h) of the pixels `disparity` can answer - those whose window, at every disparity of the range, lies inside both images -
    from libvp's plan (vp_stereo_bm_plan; no device needed); (0, 0, 0, 0) when there is none."""
    n, bs, m = _matcher(num_disparities, block_size, min_disparity)[:3]
    if not (1 <= int(w) <= MAX_SIDE and 1 <= int(h) <= MAX_SIDE):
        raise ValueError("width and height must lie in 1..4096")
    rect, geom, ws = (C.c_int32 * 4)(), (C.c_int32 * 5)(), C.c_size_t()
    _vp.check(_vp.lib().vp_stereo_bm_plan(int(w), int(h), n, bs, m, rect, C.byref(ws), geom))
    return tuple(rect)


def _disparity_dev(ctx, left, right, params):
    """both images on the device -> an int16 DeviceMat, enqueued"""
    left, right = device_image(ctx, left, 1), device_image(ctx, right, 1)
    h, w = left.shape
    out = DeviceMat(ctx, (h, w), np.int16)
    _vp.check(_vp.lib().vp_stereo_bm_dev(ctx.handle, left.dev_ptr, w, right.dev_ptr, w, w, h, *params, out.dev_ptr, 2 * w), ctx.handle)
    return out


def _depth_dev(ctx, disp, focal_px, baseline_m):
    h, w = disp.shape
    out = DeviceMat(ctx, (h, w), np.float32)
    _vp.check(_vp.lib().vp_depth_from_disparity_dev(ctx.handle, disp.dev_ptr, 2 * w, w, h, focal_px, baseline_m, out.dev_ptr, 4 * w), ctx.handle)
    return out


def disparity(left, right, num_disparities: int = 64, block_size: int = 15, min_disparity: int = 0, pre_filter_cap: int = 31, texture_threshold: int = 10,
              uniqueness_ratio: int = 15):
    """16 times the disparity of every pixel of `left`, int16, `invalid_disparity(min_disparity)` where there is no answer: outside
    `valid_rect`, where the window has too little texture, and where a second disparity is within uniqueness_ratio per cent of the
    best.  uint8 (h, w) images of one size up to 4096 x 4096; (h, w, 3) images go through bgr_to_gray first.  num_disparities a multiple
    of 16 in 16..256, block_size odd in 5..21, min_disparity in -128..128, pre_filter_cap in 1..63, uniqueness_ratio in 0..100.
    numpy in gives numpy out; if either image is a DeviceMat the result is an int16 DeviceMat that stays in HBM."""
    params = _matcher(num_disparities, block_size, min_disparity, pre_filter_cap, texture_threshold, uniqueness_ratio)
    left, right = _pair(left, right)
    ctx = _vp.default_context()
    if isinstance(left, DeviceMat) or isinstance(right, DeviceMat):
        return _disparity_dev(ctx, left, right, params)
    left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    h, w = left.shape
    out = np.empty((h, w), np.int16)
    _vp.check(_vp.lib().vp_stereo_bm_u8(ctx.handle, left.ctypes.data, right.ctypes.data, w, h, *params, out.ctypes.data), ctx.handle)
    return out


def _depth_args(disp16, focal_px, baseline_m):
    if not isinstance(disp16, (np.ndarray, DeviceMat)) or disp16.dtype != np.int16 or len(disp16.shape) != 2 or 0 in disp16.shape:
        raise TypeError("expected a non-empty int16 (h, w) disparity image")
    if max(disp16.shape) > MAX_SIDE:
        raise ValueError("the disparity image must be at most 4096 x 4096")
    return disp16, float(focal_px), float(baseline_m)


def depth_from_disparity(disp16, focal_px: float, baseline_m: float):
    """Metric depth of an int16 disparity image (16 times the disparity, as `disparity` returns it): float32 metres,
    focal_px * baseline_m * 16 / disp16 as one double quotient rounded once, and 0 where disp16 <= 0 - the `depth` plane's rule for
    pixels without an answer.  numpy in gives numpy out, a DeviceMat a DeviceMat."""
    disp16, focal_px, baseline_m = _depth_args(disp16, focal_px, baseline_m)
    ctx = _vp.default_context()
    if isinstance(disp16, DeviceMat):
        disp16.refresh_device(ctx)
        return _depth_dev(ctx, disp16, focal_px, baseline_m)
    disp16 = np.ascontiguousarray(disp16)
    h, w = disp16.shape
    out = np.empty((h, w), np.float32)
    _vp.check(_vp.lib().vp_depth_from_disparity_i16(ctx.handle, disp16.ctypes.data, w, h, focal_px, baseline_m, out.ctypes.data), ctx.handle)
    return out


def _depth_chain(match_dev, params, left, right, focal_px, baseline_m):
    """matcher, then depth, both queued; match_dev: _disparity_dev or _disparity_sgm_dev with its checked parameters"""
    left, right = _pair(left, right)
    focal_px, baseline_m = float(focal_px), float(baseline_m)
    on_device = isinstance(left, DeviceMat) or isinstance(right, DeviceMat)
    ctx = _vp.default_context()
    depth = _depth_dev(ctx, match_dev(ctx, left, right, params), focal_px, baseline_m)
    return depth if on_device else depth.host()


def stereo_depth(left, right, focal_px: float, baseline_m: float, **matcher):
    """`depth_from_disparity(disparity(left, right, **matcher), focal_px, baseline_m)` with the disparity kept in HBM between the two:
    numpy images are uploaded, both steps are queued, and only the float32 depth comes back (a DeviceMat if either image was one)."""
    return _depth_chain(_disparity_dev, _matcher(**matcher), left, right, focal_px, baseline_m)


def _int_in(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise TypeError(f"{name} must be an integer")
    if not lo <= v <= hi:
        raise ValueError(f"{name} must lie in {lo}..{hi}")
    return int(v)


def _speckle_args(disp16, max_speckle_size, max_diff, new_val):
    """everything libvp refuses of a filter_speckles call, refused here before a device is needed"""
    if not isinstance(disp16, (np.ndarray, DeviceMat)) or disp16.dtype != np.int16 or len(disp16.shape) != 2 or 0 in disp16.shape:
        raise TypeError("expected a non-empty int16 (h, w) disparity image")
    if max(disp16.shape) > MAX_SIDE:
        raise ValueError("the disparity image must be at most 4096 x 4096")
    h, w = disp16.shape
    new_val = invalid_disparity(0) if new_val is None else new_val
    return (_int_in("new_val", new_val, -32768, 32767), _int_in("max_speckle_size", max_speckle_size, 0, w * h), _int_in("max_diff", max_diff, 0, 65535))


def _speckles_dev(ctx, disp, params, out=None):
    """an int16 DeviceMat -> the filtered DeviceMat, enqueued; out: the image to write (the source itself: in place)"""
    h, w = disp.shape
    out = DeviceMat(ctx, (h, w), np.int16) if out is None else out
    _vp.check(_vp.lib().vp_filter_speckles_dev(ctx.handle, disp.dev_ptr, 2 * w, w, h, *params, out.dev_ptr, 2 * w), ctx.handle)
    return out


def filter_speckles(disp16, max_speckle_size: int, max_diff: int, new_val=None):
    """cv2.filterSpeckles as a function that returns a new image: every connected region of `disp16` (int16, 16 times the disparity, as
    `disparity` returns it) of at most max_speckle_size pixels becomes new_val.  Two pixels are linked when they are 4-neighbours,
    neither equals new_val and they differ by at most max_diff (so max_diff = 16 * speckleRange); links chain.  new_val defaults to
    `invalid_disparity(0)`.  max_speckle_size in 0..w*h (0 copies), max_diff in 0..65535.  numpy in gives numpy out, a DeviceMat a
    DeviceMat that stays in HBM."""
    params = _speckle_args(disp16, max_speckle_size, max_diff, new_val)
    ctx = _vp.default_context()
    if isinstance(disp16, DeviceMat):
        disp16.refresh_device(ctx)
        return _speckles_dev(ctx, disp16, params)
    disp16 = np.ascontiguousarray(disp16)
    h, w = disp16.shape
    out = np.empty((h, w), np.int16)
    _vp.check(_vp.lib().vp_filter_speckles_i16(ctx.handle, disp16.ctypes.data, w, h, *params, out.ctypes.data), ctx.handle)
    return out


def _normals_args(depth, focal_px, cx, cy, max_jump_m, encode):
    if not isinstance(depth, (np.ndarray, DeviceMat)) or depth.dtype != np.float32 or len(depth.shape) != 2 or 0 in depth.shape:
        raise TypeError("expected a non-empty float32 (h, w) depth image")
    if max(depth.shape) > MAX_SIDE:
        raise ValueError("the depth image must be at most 4096 x 4096")
    h, w = depth.shape
    focal_px = float(focal_px)
    cx, cy = (w - 1) / 2 if cx is None else float(cx), (h - 1) / 2 if cy is None else float(cy)
    max_jump_m = 0.0 if max_jump_m is None else float(max_jump_m)
    if not (np.isfinite(focal_px) and focal_px > 0):
        raise ValueError("focal_px must be finite and positive")
    if not (np.isfinite(cx) and np.isfinite(cy)):
        raise ValueError("cx and cy must be finite")
    if np.isnan(max_jump_m):
        raise ValueError("max_jump_m is not a number")
    return focal_px, cx, cy, max_jump_m, int(bool(encode))


def _normals_dev(ctx, depth, params):
    h, w = depth.shape
    out = DeviceMat(ctx, (h, w, 3), np.float32)
    _vp.check(_vp.lib().vp_normals_from_depth_dev(ctx.handle, depth.dev_ptr, 4 * w, w, h, *params, out.dev_ptr, 12 * w), ctx.handle)
    return out


def normals_from_depth(depth, focal_px: float, cx=None, cy=None, max_jump_m=None, encode: bool = False):
    """Surface normals of a float32 depth image in metres, float32 (h, w, 3), by this library's own definition (the vendor SDK's is
    closed).  A normal exists where the pixel and its four neighbours are inside the image with a finite depth above 0 - and, with
    max_jump_m, none of the four differs from the centre by more than it: a depth edge gives no normal.  With P the back-projection
    ((x - cx) Z / f, (y - cy) Z / f, Z), the normal is the unit vector of (P(x, y+1) - P(x, y-1)) x (P(x+1, y) - P(x-1, y)), which
    faces the camera: (0, 0, -1) for a wall square to the optical axis.  cx, cy default to the image centre ((w-1)/2, (h-1)/2).
    Without a normal the result is NaN thrice; encode=True gives the reference's `normal` plane instead, (n + 1) / 2 and 0 without a
    normal.  numpy in gives numpy out, a DeviceMat a DeviceMat."""
    params = _normals_args(depth, focal_px, cx, cy, max_jump_m, encode)
    ctx = _vp.default_context()
    if isinstance(depth, DeviceMat):
        depth.refresh_device(ctx)
        return _normals_dev(ctx, depth, params)
    depth = np.ascontiguousarray(depth)
    h, w = depth.shape
    out = np.empty((h, w, 3), np.float32)
    _vp.check(_vp.lib().vp_normals_from_depth_f32(ctx.handle, depth.ctypes.data, w, h, *params, out.ctypes.data), ctx.handle)
    return out


def stereo_planes(left, right, focal_px: float, baseline_m: float, cx=None, cy=None, speckle_window_size: int = 100, speckle_range: int = 2, max_jump_m=None,
                  **matcher):
    """The `depth` and `normal` planes of the reference's forward camera (zed_sync.py:148-149) from a rectified pair: `disparity`, then
    `filter_speckles` with max_diff = 16 * speckle_range and new_val = invalid_disparity(min_disparity) (skipped when
    speckle_window_size is 0), then `depth_from_disparity`, then `normals_from_depth(encode=True)`.  All four are queued on the device
    and nothing visits the host in between; (depth, normal) come back as DeviceMats if either image was one, else as numpy arrays.
    speckle_window_size = 100 and speckle_range = 2 are the middle of the range OpenCV's documentation recommends (50-200, 1-2);
    nothing here measured them."""
    return _planes_chain(_disparity_dev, _matcher(**matcher), left, right, focal_px, baseline_m, cx, cy, speckle_window_size, speckle_range, max_jump_m)


def _planes_chain(match_dev, params, left, right, focal_px, baseline_m, cx, cy, speckle_window_size, speckle_range, max_jump_m):
    """matcher, speckle filter, depth, normals, all queued; params[2] is min_disparity for both matchers"""
    left, right = _pair(left, right)
    focal_px, baseline_m = float(focal_px), float(baseline_m)
    h, w = left.shape
    window = _int_in("speckle_window_size", speckle_window_size, 0, w * h)
    diff = 16 * _int_in("speckle_range", speckle_range, 0, 4095)
    nparams = _normals_args(np.empty((1, 1), np.float32), focal_px, (w - 1) / 2 if cx is None else cx, (h - 1) / 2 if cy is None else cy, max_jump_m, True)
    on_device = isinstance(left, DeviceMat) or isinstance(right, DeviceMat)
    ctx = _vp.default_context()
    disp = match_dev(ctx, left, right, params)
    if window:
        disp = _speckles_dev(ctx, disp, (invalid_disparity(params[2]), window, diff), out=disp)
    depth = _depth_dev(ctx, disp, focal_px, baseline_m)
    normal = _normals_dev(ctx, depth, nparams)
    return (depth, normal) if on_device else (depth.host(), normal.host())


_SGM_RANGES = (("num_disparities", 16, 256), ("block_size", 1, 9), ("min_disparity", -128, 128), ("pre_filter_cap", 1, 63), ("p1", 0, 65535), ("p2", 0, 65535),
               ("uniqueness_ratio", 0, 100), ("disp12_max_diff", -1, 255), ("paths", 4, 8))
SGM_MAX_SUM = 65535


def _matcher_sgm(num_disparities=64, block_size=5, min_disparity=0, pre_filter_cap=31, p1=None, p2=None, uniqueness_ratio=10, disp12_max_diff=1, paths=8):
    """the nine checked parameters, in the order of the C entries; everything libvp refuses is refused here, before a device is needed"""
    given = [num_disparities, block_size, min_disparity, pre_filter_cap, p1, p2, uniqueness_ratio, disp12_max_diff, paths]
    for (name, _, _), v in zip(_SGM_RANGES, given):
        if not (v is None and name in ("p1", "p2")) and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
            raise TypeError(f"{name} must be an integer")
    if given[4] is None:
        given[4] = 8 * int(block_size) ** 2
    if given[5] is None:
        given[5] = 32 * int(block_size) ** 2
    out = []
    for (name, lo, hi), v in zip(_SGM_RANGES, given):
        if not lo <= v <= hi:
            raise ValueError(f"{name} must lie in {lo}..{hi}")
        out.append(int(v))
    n, bs, _, cap, p1, p2, _, _, paths = out
    if n % 16:
        raise ValueError("num_disparities must be a multiple of 16")
    if bs % 2 == 0:
        raise ValueError("block_size must be odd")
    if paths not in (4, 8):
        raise ValueError("paths must be 4 or 8")
    if p1 > p2:
        raise ValueError("p1 must not exceed p2")
    if paths * (2 * cap * bs * bs + p2) > SGM_MAX_SUM:
        raise ValueError(f"paths * (2 * pre_filter_cap * block_size^2 + p2) must not exceed {SGM_MAX_SUM}: the summed path costs are 16-bit")
    return tuple(out)


def valid_rect_sgm(w: int, h: int, num_disparities: int = 64, block_size: int = 5, min_disparity: int = 0):
    """(x, y, w, h) of the pixels `disparity_sgm` can answer, from libvp's plan (vp_stereo_sgm_plan; no device needed): `valid_rect`'s
    rule at this block size; (0, 0, 0, 0) when there is none."""
    n, bs, m = _matcher_sgm(num_disparities, block_size, min_disparity, p1=0, p2=0)[:3]
    if not (1 <= int(w) <= MAX_SIDE and 1 <= int(h) <= MAX_SIDE):
        raise ValueError("width and height must lie in 1..4096")
    rect, geom, ws = (C.c_int32 * 4)(), (C.c_int32 * 15)(), C.c_size_t()
    _vp.check(_vp.lib().vp_stereo_sgm_plan(int(w), int(h), n, bs, m, 8, rect, C.byref(ws), geom))
    return tuple(rect)


SGM_MAX_WORKSPACE = 1 << 32


def _sgm_pair(left, right, params):
    """`_pair`, and the one refusal of libvp's that depends on the size: the workspace of the call"""
    left, right = _pair(left, right)
    h, w = left.shape
    rect, geom, ws = (C.c_int32 * 4)(), (C.c_int32 * 15)(), C.c_size_t()
    if _vp.lib().vp_stereo_sgm_plan(w, h, params[0], params[1], params[2], params[8], rect, C.byref(ws), geom) != 0:
        raise ValueError(f"the workspace of this call would exceed {SGM_MAX_WORKSPACE} bytes (4 GiB): {w} x {h} at {params[0]} disparities")
    return left, right


def _disparity_sgm_dev(ctx, left, right, params):
    """both images on the device -> an int16 DeviceMat, enqueued"""
    left, right = device_image(ctx, left, 1), device_image(ctx, right, 1)
    h, w = left.shape
    out = DeviceMat(ctx, (h, w), np.int16)
    _vp.check(_vp.lib().vp_stereo_sgm_dev(ctx.handle, left.dev_ptr, w, right.dev_ptr, w, w, h, *params, out.dev_ptr, 2 * w), ctx.handle)
    return out


def disparity_sgm(left, right, num_disparities: int = 64, block_size: int = 5, min_disparity: int = 0, pre_filter_cap: int = 31, p1=None, p2=None,
                  uniqueness_ratio: int = 10, disp12_max_diff: int = 1, paths: int = 8):
    """16 times the disparity of every pixel of `left` by semi-global matching, int16, `invalid_disparity(min_disparity)` where there
    is no answer: outside `valid_rect_sgm`, where a second disparity is within uniqueness_ratio per cent of the best, and where the
    right view's answer differs from the left's by more than disp12_max_diff (-1: not checked).  The cost is `disparity`'s window sum
    of absolute differences of the prefiltered images, without a texture test; it is summed along `paths` (4 or 8) directions with the
    penalty p1 for a change of disparity by one and p2 for a larger change.  p1=None means 8 * block_size^2 and p2=None
    32 * block_size^2: the values OpenCV's documentation recommends for one channel; nothing here measured them.  uint8 (h, w) images
    of one size up to 4096 x 4096; (h, w, 3) images go through bgr_to_gray first.  num_disparities a multiple of 16 in 16..256,
    block_size odd in 1..9, min_disparity in -128..128, pre_filter_cap in 1..63, 0 <= p1 <= p2, uniqueness_ratio in 0..100,
    disp12_max_diff in -1..255, and paths * (2 * pre_filter_cap * block_size^2 + p2) <= 65535, which keeps the summed costs in 16 bits.
    The scratch of a call, 4 * num_disparities bytes per candidate pixel, must not exceed 4 GiB.  numpy in gives numpy out; if either
    image is a DeviceMat the result is an int16 DeviceMat that stays in HBM."""
    params = _matcher_sgm(num_disparities, block_size, min_disparity, pre_filter_cap, p1, p2, uniqueness_ratio, disp12_max_diff, paths)
    left, right = _sgm_pair(left, right, params)
    ctx = _vp.default_context()
    if isinstance(left, DeviceMat) or isinstance(right, DeviceMat):
        return _disparity_sgm_dev(ctx, left, right, params)
    left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    h, w = left.shape
    out = np.empty((h, w), np.int16)
    _vp.check(_vp.lib().vp_stereo_sgm_u8(ctx.handle, left.ctypes.data, right.ctypes.data, w, h, *params, out.ctypes.data), ctx.handle)
    return out


def stereo_depth_sgm(left, right, focal_px: float, baseline_m: float, **matcher):
    """`stereo_depth` with `disparity_sgm` as the matcher: **matcher are its parameters."""
    params = _matcher_sgm(**matcher)
    return _depth_chain(_disparity_sgm_dev, params, *_sgm_pair(left, right, params), focal_px, baseline_m)


def stereo_planes_sgm(left, right, focal_px: float, baseline_m: float, cx=None, cy=None, speckle_window_size: int = 100, speckle_range: int = 2, max_jump_m=None,
                      **matcher):
    """`stereo_planes` with `disparity_sgm` as the matcher: **matcher are its parameters; the steps after the matcher are the same."""
    params = _matcher_sgm(**matcher)
    return _planes_chain(_disparity_sgm_dev, params, *_sgm_pair(left, right, params), focal_px, baseline_m, cx, cy, speckle_window_size, speckle_range, max_jump_m)
