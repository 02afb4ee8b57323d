"""The statement of cv2.matchTemplate as this library computes it, in numpy with int64 and float64 only.

Per result pixel the sums C = sum I T, S2 = sum I^2 and S1_c = sum I per channel, over the window and all channels, are exact integers,
as are T2 = sum T^2 and T1_c per template.  The steps after them follow OpenCV 4.x common_matchTemplate (imgproc/src/templmatch.cpp)
with its decision rules kept; only its float32 DFT correlation is replaced by the exact C.  Every division is one IEEE double division
of two exactly converted integers, every root is correctly rounded, the order of operations is fixed, and the value is rounded to
float32 once.  Under N cn <= 65536 (N = tw th) every sum is below 2^32 and N times a sum below 2^48, so all conversions are exact."""
import numpy as np

SQDIFF, SQDIFF_NORMED, CCORR, CCORR_NORMED, CCOEFF, CCOEFF_NORMED = range(6)
METHODS = (SQDIFF, SQDIFF_NORMED, CCORR, CCORR_NORMED, CCOEFF, CCOEFF_NORMED)
NORMED = (SQDIFF_NORMED, CCORR_NORMED, CCOEFF_NORMED)
MAX_SIDE, MAX_ELEMS = 4096, 65536
FLT_EPSILON = float(np.finfo(np.float32).eps)


def _three(a):
    a = np.asarray(a)
    assert a.dtype == np.uint8 and a.ndim in (2, 3)
    return (a[:, :, None] if a.ndim == 2 else a).astype(np.int64)


def _window_sums(plane, tw, th):
    """sums of every th x tw window of an int64 (H, W) plane, by its integral image"""
    h, w = plane.shape
    ii = np.zeros((h + 1, w + 1), np.int64)
    ii[1:, 1:] = plane.cumsum(0).cumsum(1)
    return ii[th:, tw:] - ii[:-th, tw:] - ii[th:, :-tw] + ii[:-th, :-tw]


def sums(image, templ):
    """(C, S2, S1, T2, T1, N): C and S2 int64 (rh, rw), S1 int64 (cn, rh, rw), T2 int, T1 int64 (cn,), N int"""
    I, T = _three(image), _three(templ)
    (h, w, cn), (th, tw, tcn) = I.shape, T.shape
    assert cn == tcn and 1 <= cn <= 4 and 1 <= th <= h <= MAX_SIDE and 1 <= tw <= w <= MAX_SIDE and tw * th * cn <= MAX_ELEMS
    rh, rw = h - th + 1, w - tw + 1
    C = np.zeros((rh, rw), np.int64)
    for dy in range(th):
        for dx in range(tw):
            C += (I[dy:dy + rh, dx:dx + rw, :] * T[dy, dx, :]).sum(2)
    S2 = _window_sums((I * I).sum(2), tw, th)
    S1 = np.stack([_window_sums(I[:, :, c], tw, th) for c in range(cn)])
    return C, S2, S1, int((T * T).sum()), T.sum((0, 1)), tw * th


def finish(C, S2, S1, T2, T1, N, method):
    """steps 1 to 3: float32 (rh, rw)"""
    dn = np.float64(N)
    d_int = N * S2
    if method in (CCORR, CCORR_NORMED):
        num = C.astype(np.float64)
    elif method in (SQDIFF, SQDIFF_NORMED):
        n_int = S2 - 2 * C + T2
        assert (n_int >= 0).all()
        num = n_int.astype(np.float64)
    else:
        num = (N * C - (S1 * T1[:, None, None]).sum(0)).astype(np.float64) / dn
        d_int = d_int - (S1 * S1).sum(0)
    if method not in NORMED:
        return num.astype(np.float32)
    tn_int = N * T2 - int((T1 * T1).sum()) if method == CCOEFF_NORMED else N * T2
    if method == CCOEFF_NORMED and tn_int == 0:
        return np.ones(C.shape, np.float32)
    templ_norm = np.sqrt(np.float64(tn_int) / dn)
    assert (d_int >= 0).all()
    diff2 = d_int.astype(np.float64) / dn
    eps = np.float64(np.float32(10) * np.float32(FLT_EPSILON)) * S2.astype(np.float64)
    t = np.where(diff2 <= np.minimum(0.5, eps), 0.0, np.sqrt(diff2) * templ_norm)
    mag = np.abs(num)
    divide = mag < t
    clamp = ~divide & (mag < t * 1.125)
    out = np.full(C.shape, 1.0 if method == SQDIFF_NORMED else 0.0, np.float64)
    out[clamp] = np.where(num[clamp] > 0, 1.0, -1.0)
    out[divide] = num[divide] / t[divide]
    return out.astype(np.float32)


def branches(image, templ, method):
    """which rule of step 3 gave each pixel: 0 t = 0, 1 the division, 2 the clamp to +-1, 3 beyond 1.125 t (normed methods, tn_int != 0)"""
    C, S2, S1, T2, T1, N = sums(image, templ)
    dn = np.float64(N)
    d_int = N * S2
    if method == CCORR_NORMED:
        num = C.astype(np.float64)
    elif method == SQDIFF_NORMED:
        num = (S2 - 2 * C + T2).astype(np.float64)
    else:
        num = (N * C - (S1 * T1[:, None, None]).sum(0)).astype(np.float64) / dn
        d_int = d_int - (S1 * S1).sum(0)
    tn_int = N * T2 - int((T1 * T1).sum()) if method == CCOEFF_NORMED else N * T2
    diff2 = d_int.astype(np.float64) / dn
    eps = np.float64(np.float32(10) * np.float32(FLT_EPSILON)) * S2.astype(np.float64)
    zero = diff2 <= np.minimum(0.5, eps)
    t = np.where(zero, 0.0, np.sqrt(diff2) * np.sqrt(np.float64(tn_int) / dn))
    mag = np.abs(num)
    return np.where(zero, 0, np.where(mag < t, 1, np.where(mag < t * 1.125, 2, 3)))


def match_template(image, templ, method):
    return finish(*sums(image, templ), method)


def best_match(image, templ, method):
    """((x, y), score): the minimum for the SQDIFF methods, the maximum otherwise, the first pixel in raster order among equals"""
    r = match_template(image, templ, method)
    i = int(np.argmin(r) if method in (SQDIFF, SQDIFF_NORMED) else np.argmax(r))
    return (i % r.shape[1], i // r.shape[1]), float(r.ravel()[i])
