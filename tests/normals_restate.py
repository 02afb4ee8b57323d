"""Surface normals of a depth image, restated in numpy float64: the contract of vp_normals_from_depth_* (DESIGN.md section 4.35).  This is
this library's own definition; the vendor SDK whose `normal` plane it stands in for (zed_sync.py:114,132-137) is closed.

  * A pixel is usable iff its depth is finite and > 0.
  * A normal exists at (x, y) iff the pixel and its four neighbours (x +- 1, y), (x, y +- 1) are inside the image and usable and, when
    max_jump_m is given (> 0 and finite), each neighbour's depth differs from the centre's by at most max_jump_m, compared in double.
  * P(x, y) = ((x - cx) * Z / f, (y - cy) * Z / f, Z); du = P(x+1, y) - P(x-1, y); dv = P(x, y+1) - P(x, y-1); c = dv x du, which faces
    the camera; len = sqrt((c0*c0 + c1*c1) + c2*c2); n_i = float32(c_i / len).  Every product, sum, quotient and the root is one IEEE
    double operation rounded on its own, in exactly this order.
  * len == 0 means no normal (and so does a len that an overflow on the way made infinite or not a number).
  * Raw output: float32 (h, w, 3), NaN thrice (0x7fc00000) without a normal.  Encoded: float32(float32(n_i + 1) / 2) in float32
    arithmetic, and 0 thrice without a normal - the reference's plane.

Only + - * / and sqrt are used, which numpy's float64 and the device's double both round correctly: the GPU form is held to this bit
for bit."""
import numpy as np


def normals_from_depth(depth, focal_px, cx=None, cy=None, max_jump_m=None, encode=False):
    Zf = np.asarray(depth)
    assert Zf.dtype == np.float32 and Zf.ndim == 2
    h, w = Zf.shape
    f = np.float64(focal_px)
    cx = np.float64((w - 1) / 2 if cx is None else cx)
    cy = np.float64((h - 1) / 2 if cy is None else cy)
    guard = max_jump_m is not None and max_jump_m > 0 and np.isfinite(max_jump_m)
    out = np.zeros((h, w, 3), np.float32) if encode else np.full((h, w, 3), np.nan, np.float32)
    if h < 3 or w < 3:
        return out
    Z = Zf.astype(np.float64)
    usable = np.isfinite(Z) & (Z > 0)
    c, l, r, u, d = (slice(1, h - 1), slice(1, w - 1)), (slice(1, h - 1), slice(0, w - 2)), (slice(1, h - 1), slice(2, w)), (slice(0, h - 2), slice(1, w - 1)), \
        (slice(2, h), slice(1, w - 1))
    have = usable[c] & usable[l] & usable[r] & usable[u] & usable[d]
    with np.errstate(all="ignore"):
        if guard:
            j = np.float64(max_jump_m)
            for s in (l, r, u, d):
                have &= np.abs(Z[s] - Z[c]) <= j
        x = np.arange(1, w - 1, dtype=np.float64)[None, :]
        y = np.arange(1, h - 1, dtype=np.float64)[:, None]
        xm, xc, xp = (x - 1) - cx, x - cx, (x + 1) - cx
        ym, yc, yp = (y - 1) - cy, y - cy, (y + 1) - cy
        Zc, Zl, Zr, Zu, Zd = Z[c], Z[l], Z[r], Z[u], Z[d]
        du0, du1, du2 = xp * Zr / f - xm * Zl / f, yc * Zr / f - yc * Zl / f, Zr - Zl
        dv0, dv1, dv2 = xc * Zd / f - xc * Zu / f, yp * Zd / f - ym * Zu / f, Zd - Zu
        c0, c1, c2 = dv1 * du2 - dv2 * du1, dv2 * du0 - dv0 * du2, dv0 * du1 - dv1 * du0
        length = np.sqrt((c0 * c0 + c1 * c1) + c2 * c2)
        have &= (length > 0) & np.isfinite(length)
        n = np.stack([c0 / length, c1 / length, c2 / length], axis=-1).astype(np.float32)
        if encode:
            n = ((n + np.float32(1)) / np.float32(2)).astype(np.float32)
    inner = out[1:h - 1, 1:w - 1]
    inner[have] = n[have]
    return out
