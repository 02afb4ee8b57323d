"""The statement of cv2.Sobel / Scharr / Laplacian / spatialGradient / convertScaleAbs on uint8 sources with scale = 1, delta = 0
(alpha = 1, beta = 0), in numpy: the oracle of tests/test_gpu_deriv.py.  The product never imports this file.

  result = saturate_cast<ddepth>( sum over the kernel of  k[i][j] * ext[y + i - ry][x + j - rx] )      per channel, in int64

where ext is the source extended by cv::borderInterpolate (explicit index maps below, -1 = the constant border's 0) and k is the outer
product of the unnormalised integer taps of cv::getDerivKernels.  Every OpenCV path produces this integer before its cast: the 8U->16S
path sums in int32, the others in floats whose partial sums stay below 64 * 64 * 255 < 2^24.  Laplacian 5 and 7 are Sobel(2,0,k) +
Sobel(0,2,k); at 5 OpenCV keeps each term in int16, and each term is at most 64 * 255 = 16,320 in magnitude there (taps [1 0 -2 0 1]
and [1 4 6 4 1]: sums of magnitudes 4 and 16), so those intermediates change nothing."""
import numpy as np

CV_8U, CV_16S, CV_32F, CV_64F = 0, 3, 5, 6
BORDER_CONSTANT, BORDER_REPLICATE, BORDER_REFLECT, BORDER_WRAP, BORDER_REFLECT_101, BORDER_ISOLATED = 0, 1, 2, 3, 4, 16
DTYPES = {CV_8U: np.uint8, CV_16S: np.int16, CV_32F: np.float32, CV_64F: np.float64}


def border_index(p, n, border):
    """cv::borderInterpolate, loop and all; -1 for BORDER_CONSTANT"""
    if 0 <= p < n:
        return p
    if border == BORDER_REPLICATE:
        return 0 if p < 0 else n - 1
    if border == BORDER_CONSTANT:
        return -1
    assert border in (BORDER_REFLECT, BORDER_REFLECT_101)
    if n == 1:
        return 0
    delta = 1 if border == BORDER_REFLECT_101 else 0
    while not 0 <= p < n:
        p = -p - 1 + delta if p < 0 else n - 1 - (p - n) - delta
    return p


def deriv_taps(n, order):
    """cv::getSobelKernels for one axis: n - 1 - order convolutions of [1 1], then `order` of [-1 1]"""
    assert n > order >= 0
    t = np.array([1], np.int64)
    for _ in range(n - 1 - order):
        t = np.convolve(t, [1, 1])
    for _ in range(order):
        t = np.convolve(t, [-1, 1])
    return t


def sobel_kernel(dx, dy, ksize):
    """(column taps, row taps) of cv2.Sobel; ksize -1 is Scharr"""
    if ksize == -1:
        return scharr_kernel(dx, dy)
    assert 0 <= dx <= 2 and 0 <= dy <= 2 and dx + dy > 0 and ksize in (1, 3, 5, 7)
    kx = deriv_taps(3 if (ksize == 1 and dx > 0) else ksize, dx)
    ky = deriv_taps(3 if (ksize == 1 and dy > 0) else ksize, dy)
    return ky, kx


def scharr_kernel(dx, dy):
    assert dx >= 0 and dy >= 0 and dx + dy == 1
    d, s = np.array([-1, 0, 1], np.int64), np.array([3, 10, 3], np.int64)
    return (s, d) if dx else (d, s)


def laplacian_kernel(ksize):
    """the 2-D kernel of cv2.Laplacian"""
    if ksize == 1:
        return np.array([[0, 1, 0], [1, -4, 1], [0, 1, 0]], np.int64)
    if ksize == 3:
        return np.array([[2, 0, 2], [0, -8, 0], [2, 0, 2]], np.int64)
    assert ksize in (5, 7)
    d2, s = deriv_taps(ksize, 2), deriv_taps(ksize, 0)
    return np.outer(s, d2) + np.outer(d2, s)


def extend(img, ry, rx, border):
    """the source with ry rows and rx pixels of border on every side, int64"""
    border &= ~BORDER_ISOLATED
    h, w = img.shape[:2]
    ym = np.array([border_index(y, h, border) for y in range(-ry, h + ry)])
    xm = np.array([border_index(x, w, border) for x in range(-rx, w + rx)])
    ext = img.astype(np.int64)[np.maximum(ym, 0)][:, np.maximum(xm, 0)]
    ext[ym < 0] = 0
    ext[:, xm < 0] = 0
    return ext


def correlate(img, k2d, border):
    """int64 correlation of every channel with k2d, anchored at its centre"""
    k2d = np.asarray(k2d, np.int64)
    kh, kw = k2d.shape
    h, w = img.shape[:2]
    ext = extend(img, kh // 2, kw // 2, border)
    acc = np.zeros(img.shape, np.int64)
    for i in range(kh):
        for j in range(kw):
            if k2d[i, j]:
                acc += k2d[i, j] * ext[i:i + h, j:j + w]
    return acc


def saturate(acc, ddepth):
    if ddepth in (-1, CV_8U):
        return np.clip(acc, 0, 255).astype(np.uint8)
    if ddepth == CV_16S:
        return np.clip(acc, -32768, 32767).astype(np.int16)
    return acc.astype(DTYPES[ddepth])


def sobel_restate(img, ddepth, dx, dy, ksize=3, border=BORDER_REFLECT_101):
    ky, kx = sobel_kernel(dx, dy, ksize)
    return saturate(correlate(img, np.outer(ky, kx), border), ddepth)


def scharr_restate(img, ddepth, dx, dy, border=BORDER_REFLECT_101):
    ky, kx = scharr_kernel(dx, dy)
    return saturate(correlate(img, np.outer(ky, kx), border), ddepth)


def laplacian_restate(img, ddepth, ksize=1, border=BORDER_REFLECT_101):
    return saturate(correlate(img, laplacian_kernel(ksize), border), ddepth)


def spatial_gradient_restate(img, border=BORDER_REFLECT_101):
    assert img.ndim == 2 and border in (BORDER_REFLECT_101, BORDER_REPLICATE)
    return sobel_restate(img, CV_16S, 1, 0, 3, border), sobel_restate(img, CV_16S, 0, 1, 3, border)


def convert_scale_abs_restate(src):
    """saturate_cast<uchar>(|v|): floats are rounded half to even first; NaN gives 0"""
    src = np.asarray(src)
    if src.dtype.kind == "f":
        a = np.rint(np.abs(src.astype(np.float64)))
        a[np.isnan(a)] = 0
    else:
        a = np.abs(src.astype(np.int64))
    return np.clip(a, 0, 255).astype(np.uint8)
