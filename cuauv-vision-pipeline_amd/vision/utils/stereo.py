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

The head and the tail (libvp vp_rectify.hip): `stereo_rectify` is the calibration-time geometry (Bouguet's
algorithm in the shape of cv2.stereoRectify, host float64, the library's own statement), `rectify_pair` turns both raw eyes into the
matcher's grey pair in one launch, byte for byte as tests/rectify_restate.py states it, `reproject_to_3d` makes XYZ points of a
disparity image, bit for bit, and `StereoRig` ties a calibration to the chain: from one raw side-by-side frame to `depth`, `normal`
and points, everything in HBM.

The quantity a mission consumes (libvp vp_plane.hip): `fit_plane` finds one plane through the usable points
of an image by RANSAC - normal, distance, inlier count and inlier mask - bit for bit as tests/plane_restate.py states the search;
`fit_planes` peels several; `StereoRig.fit_plane` searches in disparity space, where stereo noise is uniform, and answers in metres;
`plane_distance` and `plane_angles` read a result.

How the scene moved between two frames (libvp vp_rigid.hip): `fit_rigid` finds one rigid motion
q = R p + t through paired 3-D points by RANSAC, bit for bit as tests/rigid_restate.py states the search, with the distance taken in
metres or as a stereo rig sees it; `rigid_from_tracks` takes its pairs from two point images at the ends of point tracks;
`StereoRig.ego_motion` runs it from two disparity images.
"""
import ctypes as C
import dataclasses

import numpy as np

from vision import _vp
from vision.devmat import DeviceMat, finish_uploads
from vision.utils.helpers import device_image, error, image_source

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


# ---- the head and the tail of the stack: rectification and 3-D reprojection (libvp vp_rectify.hip) ------------
UNDISTORT_ITERATIONS = 100
CALIB_ZERO_DISPARITY = 1024
DISP_I16, DISP_F32 = 0, 1
_INT_MIN = -2 ** 31


def rodrigues(src):
    """cv2.Rodrigues without the Jacobian, float64: a rotation vector (3 numbers: the axis times the angle in radians) gives its 3x3
    matrix, a 3x3 rotation matrix gives its vector (angle in [0, pi])."""
    a = np.asarray(src, dtype=np.float64)
    if a.size == 3:
        r = a.ravel()
        theta = float(np.sqrt(r @ r))
        if theta < 1e-300:
            return np.eye(3)
        k = r / theta
        K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
        return np.cos(theta) * np.eye(3) + (1 - np.cos(theta)) * np.outer(k, k) + np.sin(theta) * K
    if a.shape != (3, 3):
        raise error("Rodrigues: a rotation vector of 3 numbers or a 3x3 matrix")
    v = np.array([a[2, 1] - a[1, 2], a[0, 2] - a[2, 0], a[1, 0] - a[0, 1]]) / 2          # the axis times sin(theta)
    s, c = float(np.sqrt(v @ v)), min(1.0, max(-1.0, (a[0, 0] + a[1, 1] + a[2, 2] - 1) / 2))
    theta = float(np.arctan2(s, c))
    if s >= 1e-8:
        return v * (theta / s)
    if c > 0:
        return v                                                                         # theta ~ sin(theta)
    # theta ~ pi: R + I = 2 k k^T; the signs of k from its largest component, the vector's direction either way
    d = np.maximum((np.diag(a) + 1) / 2, 0)
    k = np.sqrt(d)
    i = int(np.argmax(d))
    for j in range(3):
        if j != i and a[i, j] + a[j, i] < 0:
            k[j] = -k[j]
    return k * (theta / float(np.sqrt(k @ k)))


def _undistort_points(pts, K, k8, R=None, P=None):
    """Pixels of the raw image -> ideal points: the rational model inverted by UNDISTORT_ITERATIONS fixed-point iterations in double
    (x <- (x_d - tangential(x)) / radial(x), from x = x_d), then rotated by R and projected by P (3x3) where they are given."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    k1, k2, p1, p2, k3, k4, k5, k6 = k8
    x0, y0 = (pts[:, 0] - K[0, 2]) / K[0, 0], (pts[:, 1] - K[1, 2]) / K[1, 1]
    x, y = x0.copy(), y0.copy()
    for _ in range(UNDISTORT_ITERATIONS):
        r2 = x * x + y * y
        ikr = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx, dy = 2 * p1 * x * y + p2 * (r2 + 2 * x * x), p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (x0 - dx) * ikr, (y0 - dy) * ikr
    if R is not None:
        X = np.stack([x, y, np.ones_like(x)], axis=0)
        X = np.asarray(R, dtype=np.float64) @ X
        x, y = X[0] / X[2], X[1] / X[2]
    if P is not None:
        x, y = P[0, 0] * x + P[0, 2], P[1, 1] * y + P[1, 2]
    return np.stack([x, y], axis=-1)


def _grid_rectangles(K, k8, R, P, size, n=9):
    """inner and outer rectangle (x0, y0, x1, y1) of the n x n grid of raw pixels after undistortion, rotation and projection"""
    w, h = size
    gx, gy = np.meshgrid(np.arange(n) * (w - 1) / (n - 1), np.arange(n) * (h - 1) / (n - 1))
    p = _undistort_points(np.stack([gx.ravel(), gy.ravel()], axis=-1), K, k8, R, P).reshape(n, n, 2)
    inner = (p[:, 0, 0].max(), p[0, :, 1].max(), p[:, -1, 0].min(), p[-1, :, 1].min())
    outer = (p[..., 0].min(), p[..., 1].min(), p[..., 0].max(), p[..., 1].max())
    return inner, outer


def _taps_inside(K, d, R, P, src_size, new_size):
    """bool (h, w) of the rectified image: all four bilinear taps of the pixel, as the fixed tables place them, lie inside the source"""
    from vision.utils import transform as _transform
    u, v = _transform._undistort_coords("stereoRectify", K, d, R, P, new_size)
    xy, _ = _transform._fixed_from_double(u, v)
    sx, sy = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
    return (sx >= 0) & (sx + 1 <= src_size[0] - 1) & (sy >= 0) & (sy + 1 <= src_size[1] - 1)


def _valid_roi(inside, x0, y0, x1, y1):
    """(x, y, w, h): the pixels of [x0, x1] x [y0, y1] (real numbers), shrunk edge by edge until every pixel of it is `inside`"""
    H, W = inside.shape
    xa, ya, xb, yb = max(int(np.ceil(x0)), 0), max(int(np.ceil(y0)), 0), min(int(np.floor(x1)), W - 1), min(int(np.floor(y1)), H - 1)
    while xa <= xb and ya <= yb:
        bad = ~inside[ya:yb + 1, xa:xb + 1]
        if not bad.any():
            return int(xa), int(ya), int(xb - xa + 1), int(yb - ya + 1)
        edges = (bad[:, 0].sum(), bad[0].sum(), bad[:, -1].sum(), bad[-1].sum())
        if not any(edges):
            edges = (1, 1, 1, 1)
        worst = max(edges)
        xa, ya, xb, yb = xa + (edges[0] == worst), ya + (edges[1] == worst), xb - (edges[2] == worst), yb - (edges[3] == worst)
    return 0, 0, 0, 0


def stereo_rectify(K1, d1, K2, d2, size, R, T, zero_disparity: bool = True, alpha: float = -1, new_size=None):
    """The rectifying rotations and projections of a calibrated pair by Bouguet's algorithm, in the shape of cv2.stereoRectify:
    (R1, R2, P1, P2, Q, roi1, roi2), float64 on the host; run once per calibration.  R, T take points of the first camera to the
    second (X2 = R X1 + T); size = (width, height) of the raw images, new_size of the rectified ones (default: size).

      1. half the relative rotation goes to each camera (r = rodrigues(-rodrigues(R) / 2));
      2. a second rotation takes the rotated baseline t = r T onto the x axis, or onto the y axis when |t.y| >= |t.x| (a vertical rig);
         R1 = w r^T, R2 = w r;
      3. the focal length is the mean of the two cameras' (fy for a horizontal rig, fx for a vertical one);
      4. each principal point centres the four undistorted image corners; with zero_disparity both cameras share the mean of the
         two, otherwise only the coordinate across the baseline is shared;
      5. alpha scales the result about the principal points: 0 makes the inner rectangle of a 9 x 9 grid of undistorted points fill
         the rectified image (no invalid pixel), 1 makes the outer rectangle fit (no source pixel lost), values between blend the two
         scales, -1 keeps the scale - times new_size / size across the baseline when new_size is given;
      6. roi1, roi2 = (x, y, w, h): the inner rectangle in rectified pixels, shrunk until all four bilinear taps of every pixel lie
         inside the source.

    Q takes (x, y, disparity, 1) of the first rectified image to homogeneous points in the first rectified camera's frame
    (`reproject_to_3d`).  Distortion: the 8-coefficient rational model of cv2 (4, 5 or 8 numbers); thin-prism and tilt coefficients
    raise, as everywhere in this library.  Distortion is inverted by 100 fixed-point iterations in double (UNDISTORT_ITERATIONS).
    The statement is this library's own after the published algorithm: bit parity with cv2 is not claimed."""
    from vision.utils import transform as _transform
    A1, k1 = _transform._camera("stereoRectify", K1, d1)
    A2, k2 = _transform._camera("stereoRectify", K2, d2)
    try:
        w, h = int(size[0]), int(size[1])
        nw, nh = (w, h) if new_size is None else (int(new_size[0]), int(new_size[1]))
    except (TypeError, ValueError, IndexError):
        raise error("stereoRectify: the sizes must be (width, height)") from None
    if w <= 0 or h <= 0 or nw <= 0 or nh <= 0:
        raise error("stereoRectify: the sizes must be positive")
    R = np.asarray(R, dtype=np.float64)
    if R.size == 3:
        R = rodrigues(R)
    T = np.asarray(T, dtype=np.float64).ravel()
    if R.shape != (3, 3) or not np.isfinite(R).all() or np.abs(R.T @ R - np.eye(3)).sum(axis=1).max() > 1e-6:
        raise error("stereoRectify: R must be a finite orthonormal 3x3 matrix")
    if T.shape != (3,) or not np.isfinite(T).all() or not T.any():
        raise error("stereoRectify: T must be three finite numbers, not all zero")
    alpha = float(alpha)
    if not (alpha == -1 or 0 <= alpha <= 1):
        raise error("stereoRectify: alpha must be -1 or lie in 0..1")

    r = rodrigues(-0.5 * rodrigues(R))
    t = r @ T
    idx = 0 if abs(t[0]) > abs(t[1]) else 1
    uu = np.zeros(3)
    uu[idx] = 1.0 if t[idx] > 0 else -1.0
    ww = np.cross(t, uu)
    nww = float(np.sqrt(ww @ ww))
    if nww > 0:
        ww = ww * (np.arccos(min(1.0, abs(t[idx]) / float(np.sqrt(t @ t)))) / nww)
    wr = rodrigues(ww)
    R1, R2 = wr @ r.T, wr @ r
    t = R2 @ T

    fc = (A1[idx ^ 1, idx ^ 1] + A2[idx ^ 1, idx ^ 1]) / 2
    corners = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], dtype=np.float64)
    cc = []
    for A, k8, Rk in ((A1, k1, R1), (A2, k2, R2)):
        p = _undistort_points(corners, A, k8, Rk) * fc
        cc.append(np.array([(w - 1) / 2, (h - 1) / 2]) - p.mean(axis=0))
    mean = (cc[0] + cc[1]) / 2
    if zero_disparity:
        cc = [mean.copy(), mean.copy()]
    else:
        cc[0][idx ^ 1] = cc[1][idx ^ 1] = mean[idx ^ 1]

    # the scale about the principal points, and the principal points in the new image
    P0 = [np.array([[fc, 0, c[0]], [0, fc, c[1]], [0, 0, 1.0]]) for c in cc]
    rects = [_grid_rectangles(A, k8, Rk, Pk, (w, h)) for A, k8, Rk, Pk in ((A1, k1, R1, P0[0]), (A2, k2, R2, P0[1]))]
    cn = [np.array([c[0] * (nw - 1) / (w - 1) if w > 1 else 0.0, c[1] * (nh - 1) / (h - 1) if h > 1 else 0.0]) for c in cc]
    if alpha < 0:
        s = (nw / w) if idx == 1 else (nh / h)
    else:
        def fit(rect, c0, c1, pick):
            x0, y0, x1, y1 = rect
            with np.errstate(divide="ignore", invalid="ignore"):
                return pick(c1[0] / (c0[0] - x0), c1[1] / (c0[1] - y0), (nw - 1 - c1[0]) / (x1 - c0[0]), (nh - 1 - c1[1]) / (y1 - c0[1]))
        s0 = max(fit(rects[k][0], cc[k], cn[k], max) for k in (0, 1))
        s1 = min(fit(rects[k][1], cc[k], cn[k], min) for k in (0, 1))
        s = float(s0 * (1 - alpha) + s1 * alpha)
        if not (np.isfinite(s) and s > 0):
            raise error("stereoRectify: the undistorted images do not surround their principal points: no scale fits")
    f = fc * s
    P1 = np.array([[f, 0, cn[0][0], 0], [0, f, cn[0][1], 0], [0, 0, 1.0, 0]])
    P2 = np.array([[f, 0, cn[1][0], 0], [0, f, cn[1][1], 0], [0, 0, 1.0, 0]])
    P2[idx, 3] = t[idx] * f
    Q = np.array([[1.0, 0, 0, -cn[0][0]], [0, 1.0, 0, -cn[0][1]], [0, 0, 0, f], [0, 0, -1.0 / t[idx], (cn[0][idx] - cn[1][idx]) / t[idx]]])
    rois = []
    for k, (A, d, Rk, Pk) in enumerate(((K1, d1, R1, P1), (K2, d2, R2, P2))):
        x0, y0, x1, y1 = rects[k][0]
        inside = _taps_inside(A, d, Rk, Pk, (w, h), (nw, nh))
        rois.append(_valid_roi(inside, (x0 - cc[k][0]) * s + cn[k][0], (y0 - cc[k][1]) * s + cn[k][1], (x1 - cc[k][0]) * s + cn[k][0], (y1 - cc[k][1]) * s + cn[k][1]))
    return R1, R2, P1, P2, Q, rois[0], rois[1]


def reprojection_matrix(focal_px: float, cx: float, cy: float, baseline_m: float, cx_right=None):
    """Q of a pair that arrives rectified: the left camera's focal length and principal point in pixels, the distance between the
    cameras in metres, and the right camera's principal column where it differs (a pair rectified without zero disparity).  With it
    `reproject_to_3d` gives X = (x - cx) Z / f, Y = (y - cy) Z / f, Z = f b / (d - (cx - cx_right)): `depth_from_disparity`'s Z."""
    focal_px, cx, cy, baseline_m = float(focal_px), float(cx), float(cy), float(baseline_m)
    cxr = cx if cx_right is None else float(cx_right)
    if not (np.isfinite(focal_px) and focal_px > 0 and np.isfinite(baseline_m) and baseline_m > 0 and np.isfinite(cx) and np.isfinite(cy) and np.isfinite(cxr)):
        raise ValueError("focal_px and baseline_m must be finite and positive, the principal point finite")
    return np.array([[1.0, 0, 0, -cx], [0, 1.0, 0, -cy], [0, 0, 0, focal_px], [0, 0, 1.0 / baseline_m, -(cx - cxr) / baseline_m]])


def _table(t, which):
    from vision.utils.transform import RemapTable
    if not isinstance(t, RemapTable) or t.nearest or t.frac is None:
        raise TypeError(f"the {which} table must be a bilinear RemapTable")
    return t


def _rectify_dev(ctx, lptr, lstride, rptr, rstride, w, h, cn, tl, tr, colour):
    """one launch (vp_rectify_pair_dev) from two device pointers, whose images the caller holds.  -> grey left, grey right[, colour left, right]"""
    oh, ow = tl.shape
    if tuple(tr.shape) != (oh, ow):
        raise ValueError("the two tables must have one size")
    if max(w, h, ow, oh) > MAX_SIDE:
        raise ValueError("the images and the tables must be at most 4096 x 4096")
    grey = [DeviceMat(ctx, (oh, ow), np.uint8) for _ in range(2)]
    col = [DeviceMat(ctx, (oh, ow) if cn == 1 else (oh, ow, cn), np.uint8) for _ in range(2)] if colour else [None, None]
    for t in (tl, tr):
        t.xy.refresh_device(ctx)
        t.frac.refresh_device(ctx)
    _vp.check(_vp.lib().vp_rectify_pair_dev(ctx.handle, lptr, lstride, rptr, rstride, w, h, cn, tl.xy.dev_ptr, tl.frac.dev_ptr, tr.xy.dev_ptr, tr.frac.dev_ptr, ow, oh,
                                            grey[0].dev_ptr, ow, grey[1].dev_ptr, ow, None if col[0] is None else col[0].dev_ptr, ow * cn,
                                            None if col[1] is None else col[1].dev_ptr, ow * cn), ctx.handle)
    return tuple(grey) + (tuple(col) if colour else ())


def _raw_eye(mat, which):
    mat, cn = image_source(mat, max_side=MAX_SIDE)
    if cn not in (1, 3, 4):
        raise ValueError(f"the {which} image must have 1, 3 (BGR) or 4 (BGRA) channels")
    return mat, cn


def rectify_pair(left, right, table_left, table_right, colour: bool = False):
    """Both raw eyes of a stereo camera to the matcher's inputs in one launch (libvp vp_rectify_pair_dev): (grey_left, grey_right), or
    with colour=True (grey_left, grey_right, colour_left, colour_right).  left, right: uint8 images of one size and 1, 3 (BGR) or 4
    (BGRA) channels; the tables: bilinear RemapTables of one size (`StereoRig` builds them).  Each colour result is
    `table.apply(eye)`; each grey result is cv2's BGR2GRAY / BGRA2GRAY of that colour result (the colour result itself for one
    channel), byte for byte.  numpy in gives numpy out; if either image is a DeviceMat the results are DeviceMats that stay in HBM."""
    tl, tr = _table(table_left, "left"), _table(table_right, "right")
    (left, cn), (right, cnr) = _raw_eye(left, "left"), _raw_eye(right, "right")
    if tuple(left.shape) != tuple(right.shape) or cn != cnr:
        raise ValueError("the left and right images must have one size and one channel count")
    on_device = isinstance(left, DeviceMat) or isinstance(right, DeviceMat)
    ctx = _vp.default_context()
    h, w = left.shape[:2]
    up = []
    try:
        dl, dr = device_image(ctx, left, 0, pending=up), device_image(ctx, right, 0, pending=up)
        out = _rectify_dev(ctx, dl.dev_ptr, w * cn, dr.dev_ptr, w * cn, w, h, cn, tl, tr, colour)
    finally:
        finish_uploads(ctx, up)
    return out if on_device else tuple(m.host() for m in out)


def _reproject_args(disp, Q, invalid):
    if not isinstance(disp, (np.ndarray, DeviceMat)) or disp.dtype not in (np.dtype(np.int16), np.dtype(np.float32)) or len(disp.shape) != 2 or 0 in disp.shape:
        raise TypeError("expected a non-empty int16 or float32 (h, w) disparity image")
    if max(disp.shape) > MAX_SIDE:
        raise ValueError("the disparity image must be at most 4096 x 4096")
    q = np.ascontiguousarray(np.asarray(Q, dtype=np.float64))
    if q.shape != (4, 4) or not (np.abs(q) <= 1e100).all():
        raise ValueError("Q must be a finite 4x4 matrix with entries of at most 1e100 in magnitude")
    kind = DISP_I16 if disp.dtype == np.int16 else DISP_F32
    if invalid is None:
        invalid = _INT_MIN
    elif kind == DISP_F32:
        raise ValueError("invalid= belongs to int16 disparities: a float32 disparity without an answer is NaN or infinite")
    else:
        invalid = _int_in("invalid", invalid, -32768, 32767)
    return q, kind, invalid


def _reproject_dev(ctx, disp, q, kind, invalid):
    h, w = disp.shape
    out = DeviceMat(ctx, (h, w, 3), np.float32)
    _vp.check(_vp.lib().vp_reproject_to_3d_dev(ctx.handle, disp.dev_ptr, disp.itemsize * w, kind, w, h, q.ctypes.data, invalid, out.dev_ptr, 12 * w), ctx.handle)
    return out


def reproject_to_3d(disp, Q, invalid=None):
    """cv2.reprojectImageTo3D by this library's conventions: the float32 (h, w, 3) points (X / W, Y / W, Z / W) of
    (X, Y, Z, W) = Q (x, y, d, 1), in double with one rounding per operation, bit for bit as tests/rectify_restate.py states it.
    disp: int16 sixteenths of a pixel, as the matchers return them (d = value / 16), or float32 pixels.  Three zeros - the `depth`
    plane's "unknown" - where an int16 pixel equals `invalid` (`invalid_disparity(min_disparity)` for a matcher's result; None: no such
    value), where W is 0 and where a float32 disparity is not finite.  numpy in gives numpy out, a DeviceMat a DeviceMat."""
    q, kind, invalid = _reproject_args(disp, Q, invalid)
    ctx = _vp.default_context()
    if isinstance(disp, DeviceMat):
        disp.refresh_device(ctx)
        return _reproject_dev(ctx, disp, q, kind, invalid)
    disp = np.ascontiguousarray(disp)
    h, w = disp.shape
    out = np.empty((h, w, 3), np.float32)
    if kind == DISP_I16:
        _vp.check(_vp.lib().vp_reproject_to_3d_i16(ctx.handle, disp.ctypes.data, w, h, q.ctypes.data, invalid, out.ctypes.data), ctx.handle)
    else:
        _vp.check(_vp.lib().vp_reproject_to_3d_f32(ctx.handle, disp.ctypes.data, w, h, q.ctypes.data, out.ctypes.data), ctx.handle)
    return out


class StereoRig:
    """A calibrated stereo pair, built once: `stereo_rectify`'s R1 R2 P1 P2 Q roi1 roi2, the rectified focal_px, cx, cy and the
    baseline_m = |T|, and the two RemapTables (initUndistortRectifyMap with R1 / P1 and R2 / P2) in HBM.  Its methods take raw frames -
    two images, or one side-by-side frame of width 2 * size[0], which is split by pointer and not copied - and run the existing chain on
    them; everything between the raw frame and the last result stays in HBM.  A DeviceMat in gives DeviceMats out, numpy gives numpy.
    Rectified with zero disparity, so depth = focal_px * baseline_m / disparity holds; a vertical rig (|T.y| largest after the
    half rotation) is refused: the matchers search along rows."""
    _MATCHERS = {"bm": (_disparity_dev, _matcher), "sgm": (_disparity_sgm_dev, _matcher_sgm)}

    def __init__(self, K1, d1, K2, d2, size, R, T, alpha: float = 0, new_size=None):
        from vision.utils import transform as _transform
        self.size = (int(size[0]), int(size[1]))
        self.new_size = self.size if new_size is None else (int(new_size[0]), int(new_size[1]))
        self.R1, self.R2, self.P1, self.P2, self.Q, self.roi1, self.roi2 = stereo_rectify(K1, d1, K2, d2, self.size, R, T, True, alpha, self.new_size)
        if self.P2[0, 3] == 0:
            raise ValueError("a vertical rig: the matchers search along rows")
        if max(self.size + self.new_size) > MAX_SIDE:
            raise ValueError("the raw and the rectified images must be at most 4096 x 4096")
        self.focal_px, self.cx, self.cy = float(self.P1[0, 0]), float(self.P1[0, 2]), float(self.P1[1, 2])
        self.baseline_m = float(abs(self.P2[0, 3]) / self.focal_px)
        self.tables = []
        for K, d, Rk, Pk in ((K1, d1, self.R1, self.P1), (K2, d2, self.R2, self.P2)):
            u, v = _transform._undistort_coords("initUndistortRectifyMap", K, d, Rk, Pk, self.new_size)
            self.tables.append(_transform.RemapTable(u.astype(np.float32), v.astype(np.float32)))

    def rectify(self, left, right=None, colour: bool = False):
        """`rectify_pair` with the rig's tables; right=None: `left` is a side-by-side frame (left eye first)."""
        if right is not None:
            (left, _), (right, _) = _raw_eye(left, "left"), _raw_eye(right, "right")
            if tuple(left.shape[:2]) != self.size[::-1] or tuple(right.shape[:2]) != self.size[::-1]:
                raise ValueError("the images do not have the rig's size")
            return rectify_pair(left, right, self.tables[0], self.tables[1], colour)
        frame, cn = _raw_eye(left, "side-by-side")
        w, h = self.size
        if tuple(frame.shape[:2]) != (h, 2 * w):
            raise ValueError("a side-by-side frame is twice the rig's width")
        ctx = _vp.default_context()
        up = []
        try:
            dev = device_image(ctx, frame, 0, pending=up)
            out = _rectify_dev(ctx, dev.dev_ptr, 2 * w * cn, dev.dev_ptr + w * cn, 2 * w * cn, w, h, cn, self.tables[0], self.tables[1], colour)
        finally:
            finish_uploads(ctx, up)
        return out if isinstance(frame, DeviceMat) else tuple(m.host() for m in out)

    def _matched(self, left, right, matcher, args):
        """(match_dev, checked parameters, rectified grey DeviceMats, results stay on the device)"""
        if matcher not in self._MATCHERS:
            raise ValueError('matcher must be "bm" or "sgm"')
        match_dev, check = self._MATCHERS[matcher]
        params = check(**args)
        on_device = isinstance(left, DeviceMat) or isinstance(right, DeviceMat)
        as_dev = lambda m: m if isinstance(m, DeviceMat) else DeviceMat.from_host(_vp.default_context(), m)
        gl, gr = self.rectify(as_dev(left), None if right is None else as_dev(right))
        if matcher == "sgm":
            gl, gr = _sgm_pair(gl, gr, params)
        return match_dev, params, gl, gr, on_device

    def disparity(self, left, right=None, matcher: str = "bm", **matcher_args):
        """`disparity` (matcher="bm") or `disparity_sgm` ("sgm") of the rectified pair: int16, 16 times the disparity."""
        match_dev, params, gl, gr, on_device = self._matched(left, right, matcher, matcher_args)
        out = match_dev(_vp.default_context(), gl, gr, params)
        return out if on_device else out.host()

    def depth(self, left, right=None, matcher: str = "bm", **matcher_args):
        """`stereo_depth` / `stereo_depth_sgm` of the rectified pair with the rig's focal length and baseline: float32 metres."""
        match_dev, params, gl, gr, on_device = self._matched(left, right, matcher, matcher_args)
        out = _depth_chain(match_dev, params, gl, gr, self.focal_px, self.baseline_m)
        return out if on_device else out.host()

    def planes(self, left, right=None, matcher: str = "bm", speckle_window_size: int = 100, speckle_range: int = 2, max_jump_m=None, **matcher_args):
        """`stereo_planes` / `stereo_planes_sgm` of the rectified pair with the rig's focal_px, cx, cy and baseline_m: (depth, normal)."""
        match_dev, params, gl, gr, on_device = self._matched(left, right, matcher, matcher_args)
        out = _planes_chain(match_dev, params, gl, gr, self.focal_px, self.baseline_m, self.cx, self.cy, speckle_window_size, speckle_range, max_jump_m)
        return out if on_device else tuple(m.host() for m in out)

    def points(self, disp, min_disparity: int = 0):
        """`reproject_to_3d` of a matcher's int16 result with the rig's Q and the matcher's invalid value: float32 (h, w, 3) metres in
        the rectified left camera's frame.  A float32 disparity image has no invalid value."""
        invalid = invalid_disparity(min_disparity) if getattr(disp, "dtype", None) == np.int16 else None
        return reproject_to_3d(disp, self.Q, invalid)

    def fit_plane(self, disp, box=None, mask=None, space: str = "disparity", threshold=None, min_disparity: int = 0, **search):
        """One plane through the surface a disparity image shows inside `box` / `mask` (`fit_plane`'s arguments; **search: max_iters,
        confidence, seed, return_mask) -> PlaneFit in metres, in the rectified left camera's frame.
        space="disparity" (the default): the search runs on the points (x, y, d) - the pixel and its disparity - with the residual
        taken along d and `threshold` in pixels of disparity (default 0.5): stereo noise is uniform there, while in metres it grows
        with Z squared, and a plane in space is a plane in (x, y, d) too.  The plane found, a row vector pi, is carried to the metric
        frame as pi Q^-1 (host float64), normalised and oriented towards the camera; `centroid` is carried through Q.  `hypothesis`
        stays in disparity space, as the search left it, and `rms` stays in pixels of disparity.  A pixel with x = y = d = 0 counts
        as unknown.
        space="metric": `fit_plane` on `self.points(disp)`, `threshold` in metres (default 0.02)."""
        if space == "metric":
            return fit_plane(self.points(disp, min_disparity), box, mask, 0.02 if threshold is None else threshold, along_z=False, **search)
        if space != "disparity":
            raise ValueError('space must be "disparity" or "metric"')
        invalid = invalid_disparity(min_disparity) if getattr(disp, "dtype", None) == np.int16 else None
        fit = fit_plane(reproject_to_3d(disp, np.eye(4), invalid), box, mask, 0.5 if threshold is None else threshold, along_z=True, **search)
        if not fit.found:
            return fit
        pi = np.append(fit.normal, fit.d) @ np.linalg.inv(self.Q)
        pi = pi / np.linalg.norm(pi[:3])
        if pi[3] < 0:
            pi = -pi
        c = self.Q @ np.append(fit.centroid, 1.0)
        return dataclasses.replace(fit, normal=pi[:3], d=float(pi[3]), centroid=c[:3] / c[3])

    def ego_motion(self, disp_prev, disp_cur, prev_pts, next_pts, status=None, space: str = "disparity", threshold=None, min_disparity: int = 0, **search):
        """How the scene moved between two frames of the rig -> RigidFit, in metres, in the rectified left camera's frame:
        `rigid_from_tracks` on `self.points()` of both disparity images and the point tracks prev_pts -> next_pts between the two
        rectified left images (`track_points`' arguments and results; status as it returns it).  The fit maps the scene's points
        from the previous frame to the current one, P_cur = R P_prev + t: for a static scene that is the previous camera's pose
        seen from the current camera.  `inverse()` of it is the current camera's pose in the previous camera's frame - how the
        vehicle moved.  space="disparity" (the default): the residual is taken in pixels and pixels of disparity with the rig's
        focal_px and baseline_m, `threshold` in pixels (default 1.0); space="metric": in metres (default 0.02).  **search:
        max_iters, confidence, seed, return_mask.  Both point images are made and used in HBM."""
        if space not in ("disparity", "metric"):
            raise ValueError('space must be "disparity" or "metric"')
        camera = (self.focal_px, self.baseline_m) if space == "disparity" else None
        if threshold is None:
            threshold = 1.0 if space == "disparity" else 0.02
        as_dev = lambda m: m if isinstance(m, DeviceMat) or not isinstance(m, np.ndarray) else DeviceMat.from_host(_vp.default_context(), np.ascontiguousarray(m))
        _track_args(prev_pts, next_pts, status)
        _rigid_args(threshold, search.get("max_iters", 1000), search.get("confidence", 0.99), search.get("seed", 0), camera)
        return rigid_from_tracks(self.points(as_dev(disp_prev), min_disparity), self.points(as_dev(disp_cur), min_disparity), prev_pts, next_pts, status,
                                 threshold=threshold, camera=camera, **search)


# ---- planes through 3-D points (libvp vp_plane.hip) ------------------------------------------------------------
PLANE_MAX_ITERS = 65536


@dataclasses.dataclass
class PlaneFit:
    """What `fit_plane` found: the plane normal . P + d = 0 with |normal| = 1 and d > 0 (the normal points from the surface towards
    the camera's side, d is the camera's distance from the plane).  found False: no plane; everything else is zero then."""
    found: bool
    normal: np.ndarray          # (3,) float64, the least-squares refit over the inliers
    d: float
    hypothesis: np.ndarray      # (4,) float64, the best three-point hypothesis of the search (bit for bit the statement's)
    centroid: np.ndarray        # (3,) float64, the inliers' mean
    rms: float                  # root mean square residual of the inliers from the refit plane
    inliers: int
    usable: int                 # points the search saw
    hypotheses: int             # hypotheses taken
    mask: object = None         # with return_mask: uint8 (h, w), 255 at every inlier; numpy for numpy in, a DeviceMat for a DeviceMat


def _plane_points(points):
    """the (h, w, 3) float32 image the library reads: an image as it is, (n, 3) points laid into rows of at most 4096, padded with zero triples"""
    if not isinstance(points, (np.ndarray, DeviceMat)) or points.dtype != np.float32 or len(points.shape) not in (2, 3) or points.shape[-1] != 3 or 0 in points.shape:
        raise TypeError("expected float32 points: an (h, w, 3) image or an (n, 3) array")
    if len(points.shape) == 3:
        if max(points.shape[:2]) > MAX_SIDE:
            raise ValueError("fit plane: the image must be 1 to 4096 pixels wide and high")
        return points, None
    n = points.shape[0]
    if n > MAX_SIDE * MAX_SIDE:
        raise ValueError("fit plane: at most 4096 x 4096 points")
    w = min(n, MAX_SIDE)
    h = (n + w - 1) // w
    flat = points.host_copy() if isinstance(points, DeviceMat) else points
    img = np.zeros((h * w, 3), np.float32)
    img[:n] = flat
    return img.reshape(h, w, 3), n


def _plane_args(shape, box, mask, threshold, max_iters, confidence, seed):
    h, w = shape[:2]
    if box is not None:
        box = np.array([_int_in("box", v, -2 ** 31, 2 ** 31 - 1) for v in box], np.int32)
        if box.shape != (4,):
            raise ValueError("box must be (x0, y0, width, height)")
        if box[2] < 1 or box[3] < 1:
            raise ValueError("fit plane: the box is empty")
        if box[0] < 0 or box[1] < 0 or box[0] > w - box[2] or box[1] > h - box[3]:
            raise ValueError("fit plane: the box leaves the image")
    if mask is not None and (not isinstance(mask, (np.ndarray, DeviceMat)) or mask.dtype != np.uint8 or tuple(mask.shape) != (h, w)):
        raise TypeError("the mask must be a uint8 image of the points' size")
    threshold, confidence = float(threshold), float(confidence)
    if not (np.isfinite(threshold) and threshold > 0):
        raise ValueError("fit plane: the threshold must be finite and above 0")
    max_iters = _int_in("max_iters", max_iters, -2 ** 31, 2 ** 31 - 1)
    if not 1 <= max_iters <= PLANE_MAX_ITERS:
        raise ValueError("fit plane: max_iters must be 1 to 65536")
    if not 0 < confidence < 1:
        raise ValueError("fit plane: the confidence must be above 0 and below 1")
    return box, threshold, max_iters, confidence, _int_in("seed", seed, 0, 2 ** 32 - 1)


def _fit_plane_dev(ctx, pts, box, mask, metric, threshold, max_iters, confidence, seed, want_mask):
    """vp_fit_plane_dev on DeviceMats -> (result (12,), counts (4,), inlier DeviceMat or None)"""
    h, w = pts.shape[:2]
    out = DeviceMat(ctx, (h, w), np.uint8, binary=True) if want_mask else None
    result, counts = np.zeros(_vp.PLANE_RESULT, np.float64), np.zeros(_vp.PLANE_COUNTS, np.int32)
    _vp.check(_vp.lib().vp_fit_plane_dev(ctx.handle, pts.dev_ptr, 12 * w, w, h, None if box is None else box.ctypes.data, None if mask is None else mask.dev_ptr, w,
                                         metric, threshold, max_iters, confidence, seed, None if out is None else out.dev_ptr, w, result.ctypes.data,
                                         counts.ctypes.data), ctx.handle)
    return result, counts, out


def _plane_fit(result, counts, mask):
    return PlaneFit(found=bool(counts[3] >= 0), normal=result[0:3].copy(), d=float(result[3]), hypothesis=result[4:8].copy(), centroid=result[8:11].copy(),
                    rms=float(result[11]), inliers=int(counts[1]), usable=int(counts[0]), hypotheses=int(counts[2]), mask=mask)


def fit_plane(points, box=None, mask=None, threshold: float = 0.02, max_iters: int = 1000, confidence: float = 0.99, seed: int = 0, along_z: bool = False,
              return_mask: bool = False):
    """One plane through the usable 3-D points of an image, by RANSAC on the GPU (libvp vp_fit_plane_*; the statement:
    tests/plane_restate.py) -> PlaneFit.  points: float32 (h, w, 3), as `reproject_to_3d` and `StereoRig.points` give them - a
    pixel whose three floats are zero (the library's "unknown") or not finite is skipped - or an (n, 3) array.  box (x0, y0, width,
    height) and mask (uint8 (h, w), numpy or DeviceMat, non-zero where a pixel may be used) select the pixels.  threshold: the
    largest distance of an inlier from the plane, in the points' unit; along_z: the distance is taken along the third axis instead of
    perpendicularly (points whose noise lives in the third coordinate, such as (x, y, disparity)).  The search is a pure function of
    its arguments and `seed`.  return_mask: PlaneFit.mask is the inlier image - numpy for numpy points, a DeviceMat for a DeviceMat,
    (h, w) of the image, or (n,) for an (n, 3) array."""
    img, n = _plane_points(points)
    if n is not None and (box is not None or mask is not None):
        raise ValueError("box and mask belong to an image of points")
    box, threshold, max_iters, confidence, seed = _plane_args(img.shape, box, mask, threshold, max_iters, confidence, seed)
    metric = _vp.PLANE_ALONG_Z if along_z else _vp.PLANE_PERP
    ctx = _vp.default_context()
    on_device = isinstance(points, DeviceMat) and n is None
    if on_device or isinstance(mask, DeviceMat):
        up = []
        try:
            if isinstance(img, DeviceMat):
                img.refresh_device(ctx)
            dp = img if isinstance(img, DeviceMat) else DeviceMat.from_host(ctx, np.ascontiguousarray(img), pending=up)
            dm = None if mask is None else device_image(ctx, mask, 1, pending=up)
            if isinstance(dm, DeviceMat):
                dm.refresh_device(ctx)
            result, counts, out = _fit_plane_dev(ctx, dp, box, dm, metric, threshold, max_iters, confidence, seed, return_mask)
        finally:
            finish_uploads(ctx, up)
        if out is not None and not on_device:
            out = out.host()
        return _plane_fit(result, counts, out)
    h, w = img.shape[:2]
    img = np.ascontiguousarray(img)
    mask = None if mask is None else np.ascontiguousarray(mask)
    out = np.empty((h, w), np.uint8) if return_mask else None
    result, counts = np.zeros(_vp.PLANE_RESULT, np.float64), np.zeros(_vp.PLANE_COUNTS, np.int32)
    _vp.check(_vp.lib().vp_fit_plane_f32(ctx.handle, img.ctypes.data, w, h, None if box is None else box.ctypes.data, None if mask is None else mask.ctypes.data, metric,
                                         threshold, max_iters, confidence, seed, None if out is None else out.ctypes.data, result.ctypes.data, counts.ctypes.data),
              ctx.handle)
    if out is not None and n is not None:
        out = out.reshape(-1)[:n]
    return _plane_fit(result, counts, out)


def fit_planes(points, k: int, min_inliers: int, box=None, mask=None, **search):
    """Up to k planes, largest first as the search finds them: after each `fit_plane` its inliers leave the candidate mask
    (candidates & ~inliers, with the device mask operators: no image visits the host), and the next fit sees the rest.  Stops at the
    first fit that finds no plane or fewer than min_inliers inliers; that fit is not returned.  points: an (h, w, 3) image, numpy or
    DeviceMat; every PlaneFit carries its mask, numpy for numpy points and a DeviceMat for a DeviceMat.  **search: `fit_plane`'s
    threshold, max_iters, confidence, seed, along_z."""
    from vision.devmat import bitwise
    k, min_inliers = _int_in("k", k, 1, 1024), _int_in("min_inliers", min_inliers, 3, 2 ** 31 - 1)
    search.pop("return_mask", None)
    img, n = _plane_points(points)
    if n is not None:
        raise ValueError("fit_planes takes an (h, w, 3) image of points")
    ctx = _vp.default_context()
    on_device = isinstance(points, DeviceMat)
    dp = points if on_device else DeviceMat.from_host(ctx, np.ascontiguousarray(img))
    h, w = img.shape[:2]
    if mask is None:
        cand = DeviceMat.from_host(ctx, np.full((h, w), 255, np.uint8), binary=True)
    else:
        _plane_args(img.shape, box, mask, 1.0, 1, 0.5, 0)
        cand = mask if isinstance(mask, DeviceMat) else DeviceMat.from_host(ctx, np.ascontiguousarray(mask))
    fits = []
    for _ in range(k):
        fit = fit_plane(dp, box, cand, return_mask=True, **search)
        if not fit.found or fit.inliers < min_inliers:
            break
        cand = bitwise(_vp.BITWISE_AND, cand, bitwise(_vp.BITWISE_NOT, fit.mask))
        fits.append(fit if on_device else dataclasses.replace(fit, mask=fit.mask.host()))
    return fits


def plane_distance(fit, point):
    """Signed distance of a point (or an (n, 3) array of points) from a PlaneFit's plane, positive on the camera's side; host float64."""
    p = np.asarray(point, np.float64)
    return p @ np.asarray(fit.normal, np.float64) + float(fit.d)


def plane_angles(fit):
    """(yaw, pitch) in radians of the direction the surface faces, -normal seen from the camera, against the optical axis +Z: yaw about
    the vertical axis (positive: the surface is turned towards +X), pitch about the horizontal one (positive: towards +Y); both 0 for
    a surface that faces the camera squarely.  Host float64."""
    n = -np.asarray(fit.normal, np.float64)
    return float(np.arctan2(n[0], n[2])), float(np.arctan2(n[1], np.hypot(n[0], n[2])))


# ---- rigid motion between paired 3-D points (libvp vp_rigid.hip) ------------------------------------------------
RIGID_MAX_PAIRS = 1 << 20


@dataclasses.dataclass
class RigidFit:
    """What `fit_rigid` found: the motion q = R p + t that carries the source points onto the destination points, R a rotation
    (det +1).  found False: no motion; everything else is zero then."""
    found: bool
    R: np.ndarray               # (3, 3) float64, the least-squares refit over the inliers
    t: np.ndarray               # (3,) float64
    hypothesis: np.ndarray      # (3, 4) float64 [R | t], the best three-pair hypothesis of the search (bit for bit the statement's)
    n_usable: int               # pairs the search saw
    n_inliers: int
    n_hypotheses: int           # hypotheses taken
    best_index: int             # index of the best hypothesis, -1 when there is none
    centroids: np.ndarray       # (2, 3) float64, the inliers' mean on the source and on the destination side
    rms: float                  # root mean square distance |R p + t - q| of the inliers, in the points' unit under both metrics
    mask: object = None         # with return_mask: uint8 (n,), 1 at every inlier pair (or track)

    @property
    def matrix(self):
        """(4, 4) float64: [R t; 0 0 0 1]"""
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = self.R, self.t
        return m

    def inverse(self):
        """The motion the other way round, p = R^T q - R^T t (the search's counts, hypothesis and mask stay as they are; the
        centroids swap)."""
        Ri = self.R.T.copy()
        return dataclasses.replace(self, R=Ri, t=-(Ri @ self.t), centroids=self.centroids[::-1].copy())


def _rigid_args(threshold, max_iters, confidence, seed, camera):
    threshold, confidence = float(threshold), float(confidence)
    if not (np.isfinite(threshold) and threshold > 0):
        raise ValueError("fit rigid: the threshold must be finite and above 0")
    focal, baseline = 0.0, 0.0
    if camera is not None:
        if len(camera) != 2:
            raise ValueError("camera must be (focal_px, baseline_m)")
        focal, baseline = float(camera[0]), float(camera[1])
        if not (np.isfinite(focal) and focal > 0):
            raise ValueError("fit rigid: focal_px must be finite and above 0")
        if not (np.isfinite(baseline) and baseline > 0):
            raise ValueError("fit rigid: the baseline must be finite and above 0")
    max_iters = _int_in("max_iters", max_iters, -2 ** 31, 2 ** 31 - 1)
    if not 1 <= max_iters <= PLANE_MAX_ITERS:
        raise ValueError("fit rigid: max_iters must be 1 to 65536")
    if not 0 < confidence < 1:
        raise ValueError("fit rigid: the confidence must be above 0 and below 1")
    metric = _vp.RIGID_EUCLID if camera is None else _vp.RIGID_DISPARITY
    return metric, threshold, focal, baseline, max_iters, confidence, _int_in("seed", seed, 0, 2 ** 32 - 1)


def _track_args(prev_pts, next_pts, status):
    """(prev float32 (n, 2), rows uint32 (n, 4): x, y, err 0, status) - the rows vp_lk_flow_dev leaves"""
    prev = np.ascontiguousarray(np.asarray(prev_pts, dtype=np.float32).reshape(-1, 2))
    cur = np.ascontiguousarray(np.asarray(next_pts, dtype=np.float32).reshape(-1, 2))
    n = len(prev)
    if len(cur) != n or not 1 <= n <= RIGID_MAX_PAIRS:
        raise ValueError("fit rigid: 1 to 1048576 tracks, as many next_pts as prev_pts")
    rows = np.zeros((n, 4), np.uint32)
    rows[:, :2] = cur.view(np.uint32)
    if status is None:
        rows[:, 3] = 1
    else:
        st = np.asarray(status).reshape(-1)
        if len(st) != n:
            raise ValueError("fit rigid: one status per track")
        rows[:, 3] = st != 0
    return prev, rows


def _rigid_fit(result, counts, mask):
    found = bool(counts[3] >= 0)
    return RigidFit(found=found, R=result[0:9].reshape(3, 3).copy(), t=result[9:12].copy(), hypothesis=np.concatenate([result[12:21].reshape(3, 3), result[21:24, None]], 1),
                    n_usable=int(counts[0]), n_inliers=int(counts[1]), n_hypotheses=int(counts[2]), best_index=int(counts[3]),
                    centroids=result[24:30].reshape(2, 3).copy(), rms=float(result[30]), mask=mask)


def fit_rigid(src, dst, threshold: float = 0.02, max_iters: int = 1000, confidence: float = 0.99, seed: int = 0, camera=None, return_mask: bool = False):
    """One rigid motion dst = R src + t through paired 3-D points, by RANSAC on the GPU (libvp vp_fit_rigid_*; the statement:
    tests/rigid_restate.py) -> RigidFit.  src, dst: float32 (n, 3); a pair with a point that is not finite or is the three zeros (the
    library's "unknown") is skipped.  threshold: the largest distance |R p + t - q| of an inlier, in the points' unit.
    camera=(focal_px, baseline_m): the distance is taken as a rectified stereo rig of that focal length and baseline sees it - pixels
    in the image and pixels of disparity, `threshold` in pixels; points behind the camera (Z <= 0) are outliers.  Stereo noise is
    uniform there, while in metres it grows with Z squared.  The refit is least squares in the points' unit under both metrics.
    The search is a pure function of its arguments and `seed`.  return_mask: RigidFit.mask is uint8 (n,), 1 at every inlier."""
    for a in (src, dst):
        if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.ndim != 2 or a.shape[1] != 3:
            raise TypeError("expected float32 (n, 3) arrays of points")
    n = src.shape[0]
    if dst.shape[0] != n or not 1 <= n <= RIGID_MAX_PAIRS:
        raise ValueError("fit rigid: 1 to 1048576 pairs, as many dst as src")
    metric, threshold, focal, baseline, max_iters, confidence, seed = _rigid_args(threshold, max_iters, confidence, seed, camera)
    ctx = _vp.default_context()
    src, dst = np.ascontiguousarray(src), np.ascontiguousarray(dst)
    out = np.empty(n, np.uint8) if return_mask else None
    result, counts = np.zeros(_vp.RIGID_RESULT, np.float64), np.zeros(_vp.RIGID_COUNTS, np.int32)
    _vp.check(_vp.lib().vp_fit_rigid_f32(ctx.handle, src.ctypes.data, dst.ctypes.data, n, metric, threshold, focal, baseline, max_iters, confidence, seed,
                                         None if out is None else out.ctypes.data, result.ctypes.data, counts.ctypes.data), ctx.handle)
    return _rigid_fit(result, counts, out)


def rigid_from_tracks(points_prev, points_cur, prev_pts, next_pts, status=None, threshold: float = 0.02, max_iters: int = 1000, confidence: float = 0.99, seed: int = 0,
                      camera=None, return_mask: bool = False):
    """`fit_rigid` between the 3-D points two frames show at the ends of point tracks -> RigidFit of the motion from the previous
    frame's points to the current frame's.  points_prev, points_cur: float32 (h, w, 3) images of the same size, numpy or DeviceMat,
    as `reproject_to_3d` and `StereoRig.points` give them; a DeviceMat is used where it lies and no point image is downloaded.
    prev_pts, next_pts: (n, 2) pixel positions in the two images, status (n,) non-zero where a track was found - `track_points`'
    arguments and results.  A track gives a pair when its status is set, its coordinates are finite, both positions round to a
    pixel inside the image (the nearest pixel: interpolating points across a depth edge would invent some) and both points are
    known.  The mask is per track.  The other arguments are `fit_rigid`'s."""
    for a in (points_prev, points_cur):
        if not isinstance(a, (np.ndarray, DeviceMat)) or a.dtype != np.float32 or len(a.shape) != 3 or a.shape[2] != 3 or 0 in a.shape:
            raise TypeError("expected float32 (h, w, 3) images of points")
    if tuple(points_prev.shape) != tuple(points_cur.shape):
        raise ValueError("fit rigid: the two point images must have one size")
    h, w = points_prev.shape[:2]
    if max(h, w) > MAX_SIDE:
        raise ValueError("fit rigid: the images must be 1 to 4096 pixels wide and high")
    prev, rows = _track_args(prev_pts, next_pts, status)
    metric, threshold, focal, baseline, max_iters, confidence, seed = _rigid_args(threshold, max_iters, confidence, seed, camera)
    n = len(prev)
    ctx = _vp.default_context()
    result, counts = np.zeros(_vp.RIGID_RESULT, np.float64), np.zeros(_vp.RIGID_COUNTS, np.int32)
    if isinstance(points_prev, DeviceMat) or isinstance(points_cur, DeviceMat):
        up = []
        try:
            dev = []
            for a in (points_prev, points_cur):
                if isinstance(a, DeviceMat):
                    a.refresh_device(ctx)
                    dev.append(a)
                else:
                    dev.append(DeviceMat.from_host(ctx, np.ascontiguousarray(a), pending=up))
            drows = DeviceMat.from_host(ctx, rows, pending=up)
            out = DeviceMat(ctx, (n,), np.uint8) if return_mask else None
            _vp.check(_vp.lib().vp_fit_rigid_tracks_dev(ctx.handle, dev[0].dev_ptr, 12 * w, dev[1].dev_ptr, 12 * w, w, h, prev.ctypes.data, drows.dev_ptr, n, metric,
                                                        threshold, focal, baseline, max_iters, confidence, seed, None if out is None else out.dev_ptr,
                                                        result.ctypes.data, counts.ctypes.data), ctx.handle)
        finally:
            finish_uploads(ctx, up)
        return _rigid_fit(result, counts, None if out is None else out.host())
    a, b = np.ascontiguousarray(points_prev), np.ascontiguousarray(points_cur)
    out = np.empty(n, np.uint8) if return_mask else None
    _vp.check(_vp.lib().vp_fit_rigid_tracks_f32(ctx.handle, a.ctypes.data, b.ctypes.data, w, h, prev.ctypes.data, rows.ctypes.data, n, metric, threshold, focal, baseline,
                                                max_iters, confidence, seed, None if out is None else out.ctypes.data, result.ctypes.data, counts.ctypes.data),
              ctx.handle)
    return _rigid_fit(result, counts, out)
