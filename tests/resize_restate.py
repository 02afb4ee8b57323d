"""cv2.resize(src, dsize, fx=.., fy=.., interpolation=INTER_LINEAR) on 8-bit images as OpenCV 4.x imgproc/src/resize.cpp computes it
(cv::resize, cv::hal::resize, resizeGeneric_Invoker with HResizeLinear and VResizeLinear, resizeAreaFast_Invoker), restated in numpy
step by step - the statement the GPU kernels (csrc/vp_yolo.hip k_resize_u8, k_letterbox) are held to bit for bit.

Doubles are Python floats or float64 arrays (one rounding per operation, no fused multiply-add); float32 wherever the C++ code uses
float; cvRound and saturate_cast of a float or double are np.rint (half to even); cvFloor is np.floor.  The product never imports this
file."""
import numpy as np

INTER_RESIZE_COEF_BITS = 11
INTER_RESIZE_COEF_SCALE = 1 << INTER_RESIZE_COEF_BITS
DBL_EPSILON = float(np.finfo(np.float64).eps)


def saturate_int(v):
    """saturate_cast<int>(double): cvRound (half to even), then clamped to int32."""
    return int(min(max(np.rint(v), -2.0 ** 31), 2.0 ** 31 - 1))


def geometry(sw, sh, dsize=None, fx=None, fy=None):
    """cv::resize's sizes and scales -> (dw, dh, inv_scale_x, inv_scale_y).  With a dsize the inverse scales are dsize / ssize in
    double; without one (dsize None or (0, 0)) they are fx and fy as given, and dsize = saturate_cast<int>(ssize * inv_scale)."""
    if dsize is None or tuple(dsize) == (0, 0):
        inv_x, inv_y = float(fx), float(fy)
        if not (inv_x > 0 and inv_y > 0):
            raise ValueError("resize: fx and fy must be positive")
        dw, dh = saturate_int(sw * inv_x), saturate_int(sh * inv_y)
    else:
        dw, dh = int(dsize[0]), int(dsize[1])
        inv_x, inv_y = dw / sw, dh / sh          # int / int in Python: the correctly rounded double, as (double)dw / sw
    if dw <= 0 or dh <= 0:
        raise ValueError("resize: empty destination")
    return dw, dh, inv_x, inv_y


def area_fast_2(scale_x, scale_y):
    """is_area_fast with iscale_x == iscale_y == 2: where hal::resize turns INTER_LINEAR into INTER_AREA's fast path."""
    ix, iy = saturate_int(scale_x), saturate_int(scale_y)
    fast = abs(scale_x - ix) < DBL_EPSILON and abs(scale_y - iy) < DBL_EPSILON
    return fast and ix == 2 and iy == 2


def _coef(n, scale):
    """f = (float)((d + 0.5) * scale - 0.5), s = cvFloor(f), f -= s (in float) for d = 0 .. n-1."""
    d = np.arange(n, dtype=np.float64)
    f = ((d + 0.5) * np.float64(scale) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    return s, f


def _weights(f):
    """saturate_cast<short>(cbuf[k] * INTER_RESIZE_COEF_SCALE) for cbuf = (1.f - f, f)."""
    one, scale = np.float32(1), np.float32(INTER_RESIZE_COEF_SCALE)
    w0 = np.rint(((one - f).astype(np.float32) * scale).astype(np.float32)).astype(np.int64)
    w1 = np.rint((f * scale).astype(np.float32)).astype(np.int64)
    return np.stack([w0, w1], axis=1)


def column_table(dw, sw, scale_x):
    """-> (xofs, ialpha, xmax): source column (in pixels; OpenCV stores sx * cn + k, the same pixel for every channel), the two 11-bit
    weights, and the first dx whose right neighbour is past the edge.  Both edges are clamped: sx < 0 gives sx = 0, fx = 0; sx >= sw-1
    gives sx = sw-1, fx = 0."""
    sx, fx = _coef(dw, scale_x)
    lo = sx < 0
    sx[lo], fx[lo] = 0, 0
    hi = sx + 1 >= sw
    sx[hi], fx[hi] = sw - 1, 0                   # sx + ksize2 >= ssize.width; sx >= ssize.width - 1 is the same test for ksize 2
    xmax = int(np.argmax(hi)) if hi.any() else dw
    return sx, _weights(fx), xmax


def row_table(dh, scale_y):
    """-> (yofs, ibeta): the row table is NOT clamped.  yofs may be -1 at the top of an upscale, and ibeta keeps (1 - fy, fy) there
    and at the bottom; resizeGeneric_Invoker clips the two row indices (clip(sy + k, 0, sh)) only when it reads the rows."""
    sy, fy = _coef(dh, scale_y)
    return sy, _weights(fy)


def hresize(rows, xofs, ialpha, xmax):
    """HResizeLinear<uchar, int, short, 2048>: S0[sx] * a0 + S0[sx + cn] * a1 below xmax, S0[sx] * 2048 from xmax on.
    rows: (k, sw, cn) uint8 -> (k, dw, cn) int64."""
    r = rows.astype(np.int64)
    sw = r.shape[1]
    nxt = np.minimum(xofs + 1, sw - 1)
    out = r[:, xofs] * ialpha[None, :, 0, None] + r[:, nxt] * ialpha[None, :, 1, None]
    out[:, xmax:] = r[:, xofs[xmax:]] * INTER_RESIZE_COEF_SCALE
    return out


def vresize(S0, S1, ibeta):
    """VResizeLinear<uchar, int, short, FixedPtCast<int, uchar, 22>>: uchar((((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2).
    The sum never leaves 0..255 (the SIMD path saturates, the scalar one truncates; the assert says they cannot disagree)."""
    b0 = ibeta[:, 0, None, None]
    b1 = ibeta[:, 1, None, None]
    v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2
    assert v.min() >= 0 and v.max() <= 255
    return v.astype(np.uint8)


def area_fast_2x2(src, dw, dh):
    """resizeAreaFast_Invoker at scale 2 on whole 2x2 cells: (a + b + c + d + 2) >> 2 (the rounding of its SIMD path).  A destination
    that needs a partial cell (source not exactly twice the destination) is OpenCV's edge handling, not restated here."""
    sh, sw = src.shape[:2]
    if sw != 2 * dw or sh != 2 * dh:
        raise NotImplementedError("area-fast resize with a partial edge cell")
    s = src.astype(np.int64)
    return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def tables(sw, sh, dw, dh, inv_x, inv_y):
    """The generic path's tables for given inverse scales: scale = 1. / inv_scale in double."""
    scale_x, scale_y = 1.0 / inv_x, 1.0 / inv_y
    xofs, ialpha, xmax = column_table(dw, sw, scale_x)
    yofs, ibeta = row_table(dh, scale_y)
    return xofs, ialpha, xmax, yofs, ibeta


def resize(src, dsize=None, fx=None, fy=None):
    """cv2.resize(src, dsize, fx=fx, fy=fy, interpolation=INTER_LINEAR) for a uint8 (h, w) or (h, w, cn) image."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim in (2, 3) and src.size > 0
    img = src[:, :, None] if src.ndim == 2 else src
    sh, sw = img.shape[:2]
    dw, dh, inv_x, inv_y = geometry(sw, sh, dsize, fx, fy)
    if (dw, dh) == (sw, sh):
        return src.copy()                        # cv::resize: same size, plain copy (whatever fx, fy were)
    if area_fast_2(1.0 / inv_x, 1.0 / inv_y):
        out = area_fast_2x2(img, dw, dh)
    else:
        xofs, ialpha, xmax, yofs, ibeta = tables(sw, sh, dw, dh, inv_x, inv_y)
        r0 = np.clip(yofs, 0, sh - 1)
        r1 = np.clip(yofs + 1, 0, sh - 1)
        out = vresize(hresize(img[r0], xofs, ialpha, xmax), hresize(img[r1], xofs, ialpha, xmax), ibeta)
    return out[:, :, 0] if src.ndim == 2 else out

