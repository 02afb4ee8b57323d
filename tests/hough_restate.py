"""The standard Hough transform of OpenCV 4.x (imgproc/src/hough.cpp HoughLinesStandard, as cv2.HoughLines calls it: srn = stn = 0,
linesMax = INT_MAX) restated in numpy, step by step - the statement the GPU kernels (csrc/vp_hough.hip) are held to bit for bit.

Floats are float32 wherever the C++ code uses float: products and sums of float32 numpy arrays are rounded after every operation (no
fused multiply-add); cvRound of a float is np.rint (half to even); the trig tables use math.sin / math.cos (libm, in double), not
numpy's vectorised ones.  The product never imports this file."""
import math

import numpy as np

CV_PI = 3.1415926535897932384626433832795


def num_angle(min_theta, max_theta, theta_step):
    """computeNumangle: cvFloor((max - min) / step) + 1 in double, minus one when the last angle would repeat the first one + pi."""
    n = int(math.floor((max_theta - min_theta) / theta_step)) + 1
    if n > 1 and abs(CV_PI - (n - 1) * theta_step) < theta_step / 2:
        n -= 1
    return n


def geometry(w, h, rho, theta, min_theta=0.0, max_theta=CV_PI):
    """-> (rho_f, theta_f, irho, numrho, numangle): the float32 arguments and the accumulator's size."""
    rho_f, theta_f = np.float32(rho), np.float32(theta)
    irho = np.float32(1) / rho_f
    max_rho = w + h
    min_rho = -max_rho
    numrho = int(np.rint(np.float32((max_rho - min_rho) + 1) / rho_f))       # int / float in float, cvRound
    numangle = num_angle(float(min_theta), float(max_theta), float(theta_f))  # the float theta, promoted to double
    return rho_f, theta_f, irho, numrho, numangle


def trig_tables(numangle, min_theta, theta_f, irho):
    """createTrigTable: the angle accumulates in float; sin / cos in double times irho, rounded to float."""
    tab_sin = np.empty(numangle, np.float32)
    tab_cos = np.empty(numangle, np.float32)
    ang = np.float32(min_theta)
    for n in range(numangle):
        tab_sin[n] = np.float32(math.sin(float(ang)) * float(irho))
        tab_cos[n] = np.float32(math.cos(float(ang)) * float(irho))
        ang = np.float32(ang + theta_f)
    return tab_sin, tab_cos


def accumulator(img, rho, theta, min_theta=0.0, max_theta=CV_PI):
    """The (numangle + 2) x (numrho + 2) int64 vote counts (OpenCV: int32), with the geometry."""
    img = np.asarray(img)
    h, w = img.shape
    rho_f, theta_f, irho, numrho, numangle = geometry(w, h, rho, theta, min_theta, max_theta)
    rowlen = numrho + 2
    total = (numangle + 2) * rowlen
    acc = np.zeros(total, np.int64)
    if numrho >= 1:
        tab_sin, tab_cos = trig_tables(numangle, min_theta, theta_f, irho)
        ys, xs = np.nonzero(img)
        fx, fy = xs.astype(np.float32), ys.astype(np.float32)
        half = (numrho - 1) // 2                                              # numrho >= 1: C's truncation equals floor here
        step = max(1, (1 << 23) // max(1, len(xs)))
        for n0 in range(0, numangle, step):
            ns = np.arange(n0, min(numangle, n0 + step))
            v = fx[None, :] * tab_cos[ns][:, None] + fy[None, :] * tab_sin[ns][:, None]   # float32: two rounded products, one rounded add
            assert v.dtype == np.float32
            r = np.rint(v).astype(np.int64) + half
            idx = ((ns + 1)[:, None] * rowlen + r + 1).ravel()
            assert idx.size == 0 or (idx.min() >= 0 and idx.max() < total), "a vote outside the accumulator (undefined in OpenCV)"
            acc += np.bincount(idx, minlength=total)
    return acc.reshape(numangle + 2, rowlen), (rho_f, theta_f, numrho, numangle)


def peaks(acc, threshold):
    """findLocalMaximums: cell indices (`base`) and votes of the local maxima above threshold, in no particular order."""
    c = acc[1:-1, 1:-1]
    m = (c > threshold) & (c > acc[1:-1, :-2]) & (c >= acc[1:-1, 2:]) & (c > acc[:-2, 1:-1]) & (c >= acc[2:, 1:-1])
    n, r = np.nonzero(m)
    rowlen = acc.shape[1]
    base = (n + 1) * rowlen + r + 1
    return base.astype(np.int64), c[n, r]


def hough_lines(img, rho, theta, threshold, min_theta=0.0, max_theta=CV_PI):
    """cv2.HoughLines(img, rho, theta, threshold, None, 0, 0, min_theta, max_theta): (N, 1, 2) float32 or None."""
    acc, (rho_f, theta_f, numrho, numangle) = accumulator(img, rho, theta, min_theta, max_theta)
    if numrho < 1:
        return None
    base, votes = peaks(acc, threshold)
    if base.size == 0:
        return None
    order = np.lexsort((base, -votes))                  # hough_cmp_gt: votes descending, then base ascending
    base = base[order]
    rowlen = numrho + 2
    n = base // rowlen - 1                              # cvFloor(idx * (1. / (numrho + 2))) - 1, the same for every peak cell
    r = base - (n + 1) * rowlen - 1
    out = np.empty((len(base), 1, 2), np.float32)
    out[:, 0, 0] = (r.astype(np.float32) - np.float32(numrho - 1) * np.float32(0.5)) * rho_f
    out[:, 0, 1] = np.float32(min_theta) + n.astype(np.float32) * theta_f
    return out
