"""Stereo rectification and 3-D reprojection restated in numpy.  Test infrastructure only: it never calls the
library under test.

  * the forward camera model: a point in a camera's frame -> its pixel in the raw image (project, distort with the 8-coefficient
    rational model, apply the camera matrix) - what a calibration means, and what the maps of a rectification must invert;
  * the fused rectify: per eye the fixed bilinear gather of tests/remap_restate.py (INTER_LINEAR, BORDER_CONSTANT 0), every channel
    rounded, and from those rounded bytes the grey of tests/cvt_table_restate.py - both imported, not copied;
  * the reprojection, in its fixed operation order.

float64 arithmetic is numpy's element-wise IEEE arithmetic: one rounding per operation, no fused multiply-add."""
import numpy as np

import cvt_table_restate as CT
import remap_restate as RM

INT_MIN = -2 ** 31


def distort(x, y, k):
    """ideal normalised coordinates -> distorted ones; k = k1 k2 p1 p2 k3 k4 k5 k6 (missing ones 0)"""
    k = np.concatenate([np.asarray(k, np.float64).ravel(), np.zeros(8)])[:8] if k is not None else np.zeros(8)
    k1, k2, p1, p2, k3, k4, k5, k6 = k
    r2 = x * x + y * y
    kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
    return x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y


def project_raw(X, K, k):
    """points (n, 3) in a camera's frame -> (n, 2) pixels of its raw (distorted) image"""
    X = np.asarray(X, np.float64)
    K = np.asarray(K, np.float64)
    xd, yd = distort(X[:, 0] / X[:, 2], X[:, 1] / X[:, 2], k)
    return np.stack([K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]], axis=-1)


def project_rectified(X, P):
    """points (n, 3) in a rectified camera's frame -> (n, 2) pixels by the 3x4 projection P"""
    X = np.asarray(X, np.float64)
    p = (np.asarray(P, np.float64) @ np.concatenate([X, np.ones((len(X), 1))], axis=1).T).T
    return p[:, :2] / p[:, 2:3]


def rectify_eye(src, xy, frac, colour=True):
    """(grey, colour) of one eye: src (h, w) or (h, w, 3 | 4) uint8, xy int16 (oh, ow, 2), frac uint16 (oh, ow)"""
    src = np.asarray(src)
    col = RM.remap_restate(src, xy, frac, nearest=False, border="constant", value=0)
    grey = col if src.ndim == 2 else CT.bgr2gray(np.ascontiguousarray(col[:, :, :3]))
    return grey, col


def rectify_pair(left, right, table_left, table_right):
    """(grey_left, grey_right, colour_left, colour_right); a table = (xy, frac)"""
    gl, cl = rectify_eye(left, *table_left)
    gr, cr = rectify_eye(right, *table_right)
    return gl, gr, cl, cr


def reproject(disp, Q, invalid=None):
    """float32 (h, w, 3): (X / W, Y / W, Z / W) of Q (x, y, d, 1), every row ((q0 x + q1 y) + q2 d) + q3, the quotients in double and
    then rounded to float32.  int16 disparities are sixteenths of a pixel; zeros where the pixel equals `invalid`, where W == 0 and
    where a float32 disparity is not finite."""
    disp = np.asarray(disp)
    q = np.asarray(Q, np.float64).reshape(4, 4)
    h, w = disp.shape
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    if disp.dtype == np.int16:
        known = np.ones((h, w), bool) if invalid is None or invalid == INT_MIN else disp != invalid
        d = disp.astype(np.float64) / 16.0
    else:
        assert disp.dtype == np.float32 and (invalid is None or invalid == INT_MIN)
        known = np.isfinite(disp)
        d = np.where(known, disp, 0).astype(np.float64)
    rows = [((q[r, 0] * x + q[r, 1] * y) + q[r, 2] * d) + q[r, 3] for r in range(4)]
    known &= rows[3] != 0
    W = np.where(known, rows[3], 1.0)
    out = np.zeros((h, w, 3), np.float32)
    with np.errstate(over="ignore"):
        for c in range(3):
            out[:, :, c] = np.where(known, (rows[c] / W).astype(np.float32), np.float32(0))
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
