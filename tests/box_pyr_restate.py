"""The statement of cv2.boxFilter / blur, pyrDown, pyrUp and integral on uint8 sources, in numpy: the oracle of
tests/test_gpu_box_pyr.py.  The product never imports this file.  int64 arithmetic through explicit border index maps
(cv::borderInterpolate, repeated reflection and all), then the cast.

  box       sum over the kh x kw window anchored at (kw // 2, kh // 2), also for even sizes.  Unnormalised: the exact sum, saturated to
            CV_8U / CV_16S, kept in CV_32S / CV_64F, and in CV_32F only while 255 * kw * kh < 2^24.  Normalised (CV_8U only): OpenCV has
            three roundings of sum / area - a Q23 reciprocal on 16-bit sums when area <= 256 (ColumnSum<ushort, uchar>), else the float32
            product of its vector body and the double product of its scalar tail (ColumnSum<int, uchar>), both rounded half to even.  An
            area is admitted only where all that apply to it agree for every sum 0 .. 255 * area (area_is_exact); the result is that byte.
  pyr_down  ((w + 1) // 2, (h + 1) // 2); (sum_ij k_i k_j src(B(2y - 2 + i), B(2x - 2 + j)) + 128) >> 8, k = 1 4 6 4 1.
  pyr_up    (2w, 2h); even: s[x-1] + 6 s[x] + s[x+1], odd: 4 (s[x] + s[x+1]) along rows, then the same along columns with
            (.. + 32) >> 6; index -1 reads 1 (0 in a one-pixel line), index n reads n - 1.
  integral  (h + 1, w + 1[, cn]) int32, zero first row and column."""
import functools
import math

import numpy as np

from deriv_restate import (BORDER_CONSTANT, BORDER_ISOLATED, BORDER_REFLECT, BORDER_REFLECT_101, BORDER_REPLICATE, BORDER_WRAP, CV_8U, CV_16S,
                           CV_32F, CV_64F, border_index)

CV_32S = 4
BOX_BORDERS = (BORDER_REFLECT_101, BORDER_REPLICATE, BORDER_REFLECT, BORDER_CONSTANT)
PYR_DOWN_BORDERS = (BORDER_REFLECT_101, BORDER_REPLICATE, BORDER_REFLECT)
MAX_SIDE = 255


def _q23(area):
    """divScale, divDelta of ColumnSum<ushort, uchar>"""
    scalef = (1 << 23) / area
    div_scale, div_delta = math.floor(scalef), area // 2
    if scalef - div_scale < 0.5:
        div_delta += 1
    else:
        div_scale += 1
    return div_scale, div_delta


def _roundings(area):
    """every rounding of s / area OpenCV applies to a window of this area, for s = 0 .. 255 * area"""
    s = np.arange(0, 255 * area + 1, dtype=np.int64)
    if area == 1:                                   # scale == 1: OpenCV scales nothing, a 1 x 1 window is a copy
        yield s
        return
    if area <= 256:
        div_scale, div_delta = _q23(area)
        yield ((s + div_delta) * div_scale) >> 23
    yield np.rint((s.astype(np.float32) * np.float32(1.0 / area)).astype(np.float64)).astype(np.int64)
    yield np.rint(s * (1.0 / area)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def area_is_exact(area):
    """whether all of OpenCV's roundings of sum / area give the same byte for every possible sum"""
    area = int(area)
    if area < 1:
        raise ValueError("area must be positive")
    r = list(_roundings(area))
    return all(np.array_equal(r[0], x) for x in r[1:])


def _mean(acc, area):
    """the common byte: the double product rounded half to even (area_is_exact(area) holds)"""
    return np.rint(acc * (1.0 / area)).astype(np.int64)


def _window_sums(img, kw, kh, border):
    h, w = img.shape[:2]
    ax, ay = kw // 2, kh // 2
    ym = np.array([border_index(y, h, border) for y in range(-ay, h - ay + kh - 1)])
    xm = np.array([border_index(x, w, border) for x in range(-ax, w - ax + kw - 1)])
    ext = img.astype(np.int64)[np.maximum(ym, 0)][:, np.maximum(xm, 0)]
    ext[ym < 0] = 0
    ext[:, xm < 0] = 0
    rows = np.zeros((ext.shape[0],) + img.shape[1:], np.int64)
    for j in range(kw):
        rows += ext[:, j:j + w]
    acc = np.zeros(img.shape, np.int64)
    for i in range(kh):
        acc += rows[i:i + h]
    return acc


def box_filter_restate(img, ddepth=-1, kw=3, kh=3, normalize=True, border=BORDER_REFLECT_101):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    border &= ~BORDER_ISOLATED
    if border not in BOX_BORDERS:
        raise ValueError("BORDER_WRAP and other borders are not supported")
    if not (1 <= kw <= MAX_SIDE and 1 <= kh <= MAX_SIDE):
        raise ValueError("window sides are 1..255")
    acc = _window_sums(img, kw, kh, border)
    if normalize:
        if ddepth not in (-1, CV_8U):
            raise ValueError("a normalised box filter is restated for CV_8U only")
        if not area_is_exact(kw * kh):
            raise ValueError("OpenCV's roundings of sum / area disagree for area %d" % (kw * kh))
        return _mean(acc, kw * kh).astype(np.uint8)
    if ddepth in (-1, CV_8U):
        return np.clip(acc, 0, 255).astype(np.uint8)
    if ddepth == CV_16S:
        return np.clip(acc, -32768, 32767).astype(np.int16)
    if ddepth == CV_32S:
        return acc.astype(np.int32)
    if ddepth == CV_32F:
        if 255 * kw * kh >= 1 << 24:
            raise ValueError("the sum may not be exact in float32")
        return acc.astype(np.float32)
    if ddepth == CV_64F:
        return acc.astype(np.float64)
    raise ValueError("ddepth")


K5 = np.array([1, 4, 6, 4, 1], np.int64)


def pyr_down_restate(img, border=BORDER_REFLECT_101):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    border &= ~BORDER_ISOLATED
    if border not in PYR_DOWN_BORDERS:
        raise ValueError("pyrDown takes BORDER_REFLECT_101, BORDER_REPLICATE or BORDER_REFLECT")
    h, w = img.shape[:2]
    dh, dw = (h + 1) // 2, (w + 1) // 2
    s = img.astype(np.int64)
    acc = np.zeros((dh, dw) + img.shape[2:], np.int64)
    for i in range(5):
        ym = np.array([border_index(2 * y - 2 + i, h, border) for y in range(dh)])
        for j in range(5):
            xm = np.array([border_index(2 * x - 2 + j, w, border) for x in range(dw)])
            acc += K5[i] * K5[j] * s[ym][:, xm]
    return ((acc + 128) >> 8).astype(np.uint8)


def _up_index(q, n):
    return (1 if n > 1 else 0) if q < 0 else (n - 1 if q >= n else q)


def _up_axis0(s):
    """the polyphase pass along axis 0 of an int64 array: 2n values, without the shift"""
    n = s.shape[0]
    prev = s[[_up_index(i - 1, n) for i in range(n)]]
    nxt = s[[_up_index(i + 1, n) for i in range(n)]]
    out = np.empty((2 * n,) + s.shape[1:], np.int64)
    out[0::2] = prev + 6 * s + nxt
    out[1::2] = 4 * (s + nxt)
    return out


def pyr_up_restate(img, border=BORDER_REFLECT_101):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    if border & ~BORDER_ISOLATED != BORDER_REFLECT_101:
        raise ValueError("pyrUp takes BORDER_DEFAULT only")
    rows = np.swapaxes(_up_axis0(np.swapaxes(img.astype(np.int64), 0, 1)), 0, 1)       # along x
    return ((_up_axis0(rows) + 32) >> 6).astype(np.uint8)


def integral_restate(img):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    h, w = img.shape[:2]
    if 255 * w * h > 2 ** 31 - 1:
        raise ValueError("the sums do not fit int32")
    rows = np.zeros((h, w + 1) + img.shape[2:], np.int64)             # sums along each row, one pixel at a time
    for x in range(w):
        rows[:, x + 1] = rows[:, x] + img[:, x]
    out = np.zeros((h + 1, w + 1) + img.shape[2:], np.int64)          # then down the rows
    for y in range(h):
        out[y + 1] = out[y] + rows[y]
    return out.astype(np.int32)
