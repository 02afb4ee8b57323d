"""The colour k-means of DESIGN.md section 4.26, restated in numpy: what libvp's vp_kmeans_* must equal bit for bit.  Imports nothing
from the library.  Samples are the pixels of a uint8 image in raster order, centres are float32 (k, cn); distances are accumulated in
float64 in channel order, every subtract, multiply and add rounded separately (numpy never fuses them); the sums of a pass are exact
integers, so no order of addition can change them."""
import numpy as np


def samples(img):
    """(N, cn) uint8, raster order, of an (h, w) or (h, w, cn) image"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    return np.ascontiguousarray(img).reshape(img.shape[0] * img.shape[1], -1)


def assign(px, c):
    """labels (N,) int32 - the lowest k with the smallest d_k: a strict < while scanning upwards - and the exact sums n (k,) uint32,
    S1 (k, cn) uint32, S2 (k, cn) uint64"""
    c = np.asarray(c, np.float32)
    k, cn = c.shape
    p = px.astype(np.float64)
    best = lab = None
    for i in range(k):
        d = np.zeros(len(px), np.float64)
        for ch in range(cn):
            t = p[:, ch] - np.float64(c[i, ch])
            d = d + t * t
        if i == 0:
            best, lab = d, np.zeros(len(px), np.int32)
        else:
            m = d < best
            best = np.where(m, d, best)
            lab[m] = i
    n = np.bincount(lab, minlength=k).astype(np.uint32)
    s1 = np.zeros((k, cn), np.uint32)
    s2 = np.zeros((k, cn), np.uint64)
    q = px.astype(np.int64)
    for ch in range(cn):            # float64 weights hold these integer sums exactly: 65025 * 2^24 < 2^53
        s1[:, ch] = np.bincount(lab, weights=q[:, ch], minlength=k).astype(np.uint32)
        s2[:, ch] = np.bincount(lab, weights=q[:, ch] * q[:, ch], minlength=k).astype(np.uint64)
    return lab, n, s1, s2


def update(c, n, s1):
    """c' = float32(double(S1) / double(n)): one correctly rounded division, one rounding; an empty cluster keeps its centre"""
    c = np.asarray(c, np.float32)
    out = c.copy()
    full = n > 0
    out[full] = (s1[full].astype(np.float64) / n[full].astype(np.float64)[:, None]).astype(np.float32)
    return out


def shift(c_new, c):
    """max over k of the sum, in channel order, of (double(c') - double(c))^2"""
    a, b = np.asarray(c_new, np.float32).astype(np.float64), np.asarray(c, np.float32).astype(np.float64)
    s = np.zeros(len(a), np.float64)
    for ch in range(a.shape[1]):
        t = a[:, ch] - b[:, ch]
        s = s + t * t
    return float(s.max())


def compactness(c, n, s1, s2):
    """k ascending outside, ch ascending inside; per term ((S2 - (2 c) S1) + (n c) c), added in that order"""
    c = np.asarray(c, np.float32)
    total = np.float64(0.0)
    for i in range(c.shape[0]):
        for ch in range(c.shape[1]):
            cc = np.float64(c[i, ch])
            total = total + ((np.float64(s2[i, ch]) - (np.float64(2.0) * cc) * np.float64(s1[i, ch])) + (np.float64(n[i]) * cc) * cc)
    return float(total)


def run(img, c0, max_iter, eps):
    """The whole loop: dict(compactness, labels (h, w) int32, centers (k, cn) float32, counts (k,) uint32, iterations, s1, s2).  The
    returned labels, sums and compactness belong to the returned centres; after convergence one more assign runs with the new ones."""
    img = np.asarray(img)
    px = samples(img)
    c = np.array(c0, np.float32).reshape(-1, px.shape[1])
    assert 1 <= max_iter <= 100 and eps >= 0 and 1 <= len(c) <= min(256, len(px))
    it, converged = 0, False
    while True:
        lab, n, s1, s2 = assign(px, c)
        it += 1
        if it == max_iter or converged:
            break
        c_new = update(c, n, s1)
        converged = shift(c_new, c) <= np.float64(eps) * np.float64(eps)
        c = c_new
    return dict(compactness=compactness(c, n, s1, s2), labels=lab.reshape(img.shape[:2]), centers=c, counts=n, iterations=it, s1=s1, s2=s2)


def seeded(img, index):
    """the centres that the pixels at the raster indices `index` give"""
    return samples(img)[np.asarray(index)].astype(np.float32)
