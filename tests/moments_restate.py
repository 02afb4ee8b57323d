"""The statement of cv2.moments and cv2.HuMoments, in numpy and Python ints and floats: the oracle of tests/test_gpu_moments.py and
tests/test_moments_statement.py.  The product never imports this file.

  raster_moments   the ten exact integer sums  m_pq = sum x^p y^q v  (x the column, y the row; v the pixel, or 1 for a non-zero pixel
                   when `binary`), as Python ints, in cv::Moments' order  m00 m10 m01 m20 m11 m02 m30 m21 m12 m03.  OpenCV adds raster
                   moments per tile in integers and then in doubles; every term is a non-negative integer, so whenever the largest of
                   the ten sums is below 2^53 its doubles hold exactly these integers.  The library's statement for every size it
                   admits: the exact sum, rounded once to float64, then `complete`.
  label_moments    the same sums with v = 1 for each label value 0 .. nlabels - 1; a label outside that range counts nowhere.
  contour_moments  imgproc/src/moments.cpp contourMoments in float64, in its operation order, from the last point round.  The sums of
                   the higher orders pass 2^53: the order is the statement, integer arithmetic may not replace it.
  complete         completeMomentState: the 24 fields of cv2's dictionary.
  hu               cv::HuMoments."""
import math

import numpy as np

FIELDS = ("m00", "m10", "m01", "m20", "m11", "m02", "m30", "m21", "m12", "m03", "mu20", "mu11", "mu02", "mu30", "mu21", "mu12", "mu03",
          "nu20", "nu11", "nu02", "nu30", "nu21", "nu12", "nu03")
ORDER = ((0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2), (3, 0), (2, 1), (1, 2), (0, 3))       # (p, q) of m_pq
FLT_EPSILON = 1.1920928955078125e-07
DBL_EPSILON = 2.220446049250313e-16


def _sums(v):
    """the ten sums of a 2-D array of non-negative integer weights, as Python ints (object arithmetic: nothing can wrap)"""
    h, w = v.shape
    vmax = int(v.max()) if v.size else 0
    y = np.arange(h, dtype=object)
    rows = []                                                  # rows[p][y] = sum_x x^p v[y, x], Python ints
    for p in range(4):
        if vmax * w ** (p + 1) < 2 ** 62:                      # the row sums fit int64: numpy adds them, exactly
            rows.append((v.astype(np.int64) * np.arange(w, dtype=np.int64) ** p).sum(axis=1).astype(object))
        else:
            rows.append((v.astype(object) * np.arange(w, dtype=object) ** p).sum(axis=1))
    return tuple(int((rows[p] * y ** q).sum()) for p, q in ORDER)


def raster_moments(img, binary=False):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    return _sums((img != 0).astype(np.int64) if binary else img.astype(np.int64))


def label_moments(labels, nlabels):
    labels = np.asarray(labels)
    assert labels.ndim == 2 and nlabels >= 1
    out = [[0] * 10 for _ in range(nlabels)]
    ys, xs = np.nonzero((labels >= 0) & (labels < nlabels))
    for x, y, lab in zip(xs.tolist(), ys.tolist(), labels[ys, xs].tolist()):       # Python ints throughout
        row = out[lab]
        for k, (p, q) in enumerate(ORDER):
            row[k] += x ** p * y ** q
    return [tuple(r) for r in out]


def contour_moments(pts):
    """-> the ten spatial moments as Python floats"""
    pts = np.asarray(pts)
    assert pts.dtype in (np.int32, np.float32)
    pts = pts.reshape(-1, 2)
    n = len(pts)
    if n == 0:
        return (0.0,) * 10
    a00 = a10 = a01 = a20 = a11 = a02 = a30 = a21 = a12 = a03 = 0.0
    xi_1, yi_1 = float(pts[n - 1][0]), float(pts[n - 1][1])
    xi_12 = xi_1 * xi_1
    yi_12 = yi_1 * yi_1
    for i in range(n):
        xi, yi = float(pts[i][0]), float(pts[i][1])
        xi2 = xi * xi
        yi2 = yi * yi
        dxy = xi_1 * yi - xi * yi_1
        xii_1 = xi_1 + xi
        yii_1 = yi_1 + yi
        a00 += dxy
        a10 += dxy * xii_1
        a01 += dxy * yii_1
        a20 += dxy * (xi_1 * xii_1 + xi2)
        a11 += dxy * (xi_1 * (yii_1 + yi_1) + xi * (yii_1 + yi))
        a02 += dxy * (yi_1 * yii_1 + yi2)
        a30 += dxy * xii_1 * (xi_12 + xi2)
        a03 += dxy * yii_1 * (yi_12 + yi2)
        a21 += dxy * (xi_12 * (3 * yi_1 + yi) + 2 * xi * xi_1 * yii_1 + xi2 * (yi_1 + 3 * yi))
        a12 += dxy * (yi_12 * (3 * xi_1 + xi) + 2 * yi * yi_1 * xii_1 + yi2 * (xi_1 + 3 * xi))
        xi_1, yi_1, xi_12, yi_12 = xi, yi, xi2, yi2
    if abs(a00) > FLT_EPSILON:
        sg = 1.0 if a00 > 0 else -1.0
        db1_2, db1_6, db1_12, db1_24, db1_20, db1_60 = sg * 0.5, sg * (1.0 / 6), sg * (1.0 / 12), sg * (1.0 / 24), sg * (1.0 / 20), sg * (1.0 / 60)
        return (a00 * db1_2, a10 * db1_6, a01 * db1_6, a20 * db1_12, a11 * db1_24, a02 * db1_12, a30 * db1_20, a21 * db1_60, a12 * db1_60,
                a03 * db1_20)
    return (0.0,) * 10


def complete(m):
    """ten spatial moments (ints are rounded to float64 once, here) -> the 24 fields, Python floats"""
    m00, m10, m01, m20, m11, m02, m30, m21, m12, m03 = (float(v) for v in m)
    cx = cy = inv = 0.0
    if abs(m00) > DBL_EPSILON:
        inv = 1.0 / m00
        cx = m10 * inv
        cy = m01 * inv
    mu20 = m20 - m10 * cx
    mu11 = m11 - m10 * cy
    mu02 = m02 - m01 * cy
    mu30 = m30 - cx * (3 * mu20 + cx * m10)
    mu21 = m21 - cx * (2 * mu11 + cx * m01) - cy * mu20
    mu12 = m12 - cy * (2 * mu11 + cy * m10) - cx * mu02
    mu03 = m03 - cy * (3 * mu02 + cy * m01)
    s2 = inv * inv
    s3 = s2 * math.sqrt(abs(inv))
    return (m00, m10, m01, m20, m11, m02, m30, m21, m12, m03, mu20, mu11, mu02, mu30, mu21, mu12, mu03,
            mu20 * s2, mu11 * s2, mu02 * s2, mu30 * s3, mu21 * s3, mu12 * s3, mu03 * s3)


def hu(m):
    """the 24 fields (a sequence in FIELDS order, or cv2's dictionary) -> the seven invariants, Python floats"""
    if isinstance(m, dict):
        m = [m[k] for k in FIELDS]
    nu20, nu11, nu02, nu30, nu21, nu12, nu03 = (float(v) for v in m[17:24])
    t0 = nu30 + nu12
    t1 = nu21 + nu03
    q0 = t0 * t0
    q1 = t1 * t1
    n4 = 4 * nu11
    s = nu20 + nu02
    d = nu20 - nu02
    hu0 = s
    hu1 = d * d + n4 * nu11
    hu3 = q0 + q1
    hu5 = d * (q0 - q1) + n4 * t0 * t1
    t0 *= q0 - 3 * q1
    t1 *= 3 * q0 - q1
    q0 = nu30 - 3 * nu12
    q1 = 3 * nu21 - nu03
    hu2 = q0 * q0 + q1 * q1
    hu4 = q0 * t0 + q1 * t1
    hu6 = q1 * t0 - q0 * t1
    return (hu0, hu1, hu2, hu3, hu4, hu5, hu6)


def as_bytes(fields):
    """the comparison of the tests: the doubles' bytes"""
    return np.array(fields, np.float64).tobytes()
