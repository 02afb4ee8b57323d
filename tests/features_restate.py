"""A plain numpy statement of the feature operators, written from their definitions and not from the library's
source: FAST-9 (score, suppression, order), the descriptor's pattern rule and its 32 steered copies, the orientation bin, the
descriptor bits, brute-force Hamming k-nearest-neighbours with the tie order and the cross-check, the ratio test and the cap on the
number of corners.  Slow and obvious on purpose."""
import math

import numpy as np

RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
BINS, PAIRS, BORDER, DISC_R2 = 32, 256, 15, 225


# ---- FAST-9 ------------------------------------------------------------------------------------------------------------------------
def fast_m(img):
    """(h, w) int32: M at every candidate pixel (3 <= x <= w - 4, 3 <= y <= h - 4), -1000 elsewhere"""
    I = np.asarray(img).astype(np.int32)
    h, w = I.shape
    M = np.full((h, w), -1000, np.int32)
    c = I[3:h - 3, 3:w - 3]
    d = np.stack([c - I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in RING])
    best = np.full(c.shape, -1000, np.int32)
    for s in (1, -1):
        for a in range(16):
            arc = np.stack([s * d[(a + i) % 16] for i in range(9)])
            best = np.maximum(best, arc.min(axis=0))
    M[3:h - 3, 3:w - 3] = best
    return M


def fast(img, threshold, nonmax=True):
    """(xy int32 (n, 2), score int32 (n,)) in row-major order"""
    M = fast_m(img)
    corner = M > threshold
    score = np.where(corner, M - 1, 0).astype(np.int32)
    keep = corner.copy()
    if nonmax:
        h, w = score.shape
        pad = np.zeros((h + 2, w + 2), np.int32)
        pad[1:-1, 1:-1] = score
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx or dy:
                    keep &= score > pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    ys, xs = np.nonzero(keep)
    xy = np.stack([xs, ys], axis=1).astype(np.int32)
    return xy, (score[ys, xs] if nonmax else np.zeros(len(xs), np.int32)).astype(np.int32)


def top_points(xy, score, max_points):
    """the highest scores, ties to the earlier row-major position, back in row-major order"""
    if max_points is None or len(xy) <= max_points:
        return xy, score
    order = sorted(range(len(xy)), key=lambda i: (-int(score[i]), i))[:max_points]
    order = np.array(sorted(order), np.intp)
    return xy[order], score[order]


# ---- the descriptor ------------------------------------------------------------------------------------------------------------------
def _round_away(v):
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


def trig_tables():
    """(C, S): 16384 cos / sin of 2 pi k / 32, rounded half away from zero; and the least distance of |value| from a half-integer"""
    C, S, margin = [], [], 1.0
    for k in range(BINS):
        for f, out in ((math.cos, C), (math.sin, S)):
            v = 16384 * f(2 * math.pi * k / BINS)
            margin = min(margin, abs(abs(v) - math.floor(abs(v)) - 0.5))
            out.append(_round_away(v))
    return C, S, margin


def base_pattern():
    s = 0x9E3779B9
    pairs, seen = [], set()
    while len(pairs) < PAIRS:
        c = []
        for _ in range(4):
            s = (s * 1664525 + 1013904223) % 2 ** 32
            d1 = (s >> 16) % 11
            s = (s * 1664525 + 1013904223) % 2 ** 32
            d2 = (s >> 16) % 11
            c.append(d1 + d2 - 10)
        a, b = (c[0], c[1]), (c[2], c[3])
        if a == b or frozenset((a, b)) in seen:
            continue
        seen.add(frozenset((a, b)))
        pairs.append(c)
    return pairs


def _rdiv(v):
    return (1 if v >= 0 else -1) * ((abs(v) + 8192) >> 14)


def steered_patterns():
    """(32, 256, 4) int8; asserts that every coordinate stays within +-15"""
    C, S, _ = trig_tables()
    base = base_pattern()
    out = np.zeros((BINS, PAIRS, 4), np.int64)
    for k in range(BINS):
        for i, (ax, ay, bx, by) in enumerate(base):
            out[k, i] = [_rdiv(ax * C[k] - ay * S[k]), _rdiv(ax * S[k] + ay * C[k]), _rdiv(bx * C[k] - by * S[k]), _rdiv(bx * S[k] + by * C[k])]
    assert np.abs(out).max() <= BORDER
    return out.astype(np.int8)


def round_point(v):
    """the pixel of a float32 coordinate, or None when it is not finite"""
    v = float(np.float32(v))
    return int(math.floor(v + 0.5)) if math.isfinite(v) else None


def orientation_bin(img, px, py):
    m10 = m01 = 0
    for dy in range(-BORDER, BORDER + 1):
        for dx in range(-BORDER, BORDER + 1):
            if dx * dx + dy * dy <= DISC_R2:
                v = int(img[py + dy, px + dx])
                m10 += dx * v
                m01 += dy * v
    C, S, _ = trig_tables()
    vals = [m10 * C[k] + m01 * S[k] for k in range(BINS)]      # Python integers: no overflow
    return vals.index(max(vals))


def orientation_bins(img, pix):
    """orientation_bin for many pixels at once ((n, 2) int (x, y), all admissible), in int64"""
    I = np.asarray(img).astype(np.int64)
    offs = [(dx, dy) for dy in range(-BORDER, BORDER + 1) for dx in range(-BORDER, BORDER + 1) if dx * dx + dy * dy <= DISC_R2]
    assert len(offs) == 709
    m10, m01 = np.zeros(len(pix), np.int64), np.zeros(len(pix), np.int64)
    for dx, dy in offs:
        v = I[pix[:, 1] + dy, pix[:, 0] + dx]
        m10 += dx * v
        m01 += dy * v
    C, S, _ = trig_tables()
    vals = np.stack([m10 * C[k] + m01 * S[k] for k in range(BINS)], axis=1)
    return np.argmax(vals, axis=1)                             # the first maximum: ties to the lowest k


def describe(img, blurred, pts):
    """(desc uint8 (n, 32), bin uint8 (n,), status uint8 (n,)); blurred: the 7 x 7, sigma 2 GaussianBlur of img"""
    img, B = np.asarray(img), np.asarray(blurred).astype(np.int32)
    h, w = img.shape
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    n = len(pts)
    desc, bins, status = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    pix = []
    for i in range(n):
        x, y = round_point(pts[i, 0]), round_point(pts[i, 1])
        if x is None or y is None or x < BORDER or x > w - 1 - BORDER or y < BORDER or y > h - 1 - BORDER:
            continue
        status[i] = 1
        pix.append((i, x, y))
    if not pix:
        return desc, bins, status
    which = np.array([p[0] for p in pix])
    xy = np.array([[p[1], p[2]] for p in pix], np.int64)
    kb = orientation_bins(img, xy)
    pat = steered_patterns().astype(np.int64)[kb]              # (m, 256, 4)
    a = B[xy[:, 1, None] + pat[:, :, 1], xy[:, 0, None] + pat[:, :, 0]]
    b = B[xy[:, 1, None] + pat[:, :, 3], xy[:, 0, None] + pat[:, :, 2]]
    desc[which] = np.packbits(a < b, axis=1, bitorder="little")
    bins[which] = kb
    return desc, bins, status


# ---- matching ------------------------------------------------------------------------------------------------------------------------
_POP = np.array([bin(v).count("1") for v in range(256)], np.int32)


def hamming_matrix(query, train):
    query, train = np.asarray(query, np.uint8), np.asarray(train, np.uint8)
    out = np.zeros((len(query), len(train)), np.int32)
    for c in range(query.shape[1]):
        out += _POP[query[:, c, None] ^ train[None, :, c]]
    return out


def hamming_knn(query, train, k, cross_check=False):
    """(idx, dist) int32 (nq, k): the first k train rows by (distance, index); -1 / -1 beyond nt; cross_check (k = 1) clears idx where
    the train row's best query by (distance, query index) is another"""
    nq, nt = len(query), len(train)
    idx, dist = np.full((nq, k), -1, np.int32), np.full((nq, k), -1, np.int32)
    if nq == 0 or nt == 0:
        return idx, dist
    d = hamming_matrix(query, train)
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    m = order.shape[1]
    idx[:, :m] = order
    dist[:, :m] = np.take_along_axis(d, order, axis=1)
    if cross_check:
        assert k == 1
        best_query = np.argmin(d, axis=0)                      # the first minimum: ties to the lowest query index
        idx[best_query[idx[:, 0]] != np.arange(nq), 0] = -1
    return idx, dist


def ratio_test(idx, dist, ratio=0.7):
    keep = [q for q in range(len(idx)) if idx[q, 0] >= 0 and idx[q, 1] >= 0 and float(dist[q, 0]) < ratio * float(dist[q, 1])]
    keep = np.array(keep, np.intp)
    return keep, idx[keep, 0].astype(np.intp)


def perspective(H, pts):
    p = np.asarray(pts, np.float64).reshape(-1, 2)
    w = 1.0 / (H[2, 0] * p[:, 0] + H[2, 1] * p[:, 1] + H[2, 2])        # cv2 multiplies by the reciprocal
    return np.stack([(H[0, 0] * p[:, 0] + H[0, 1] * p[:, 1] + H[0, 2]) * w, (H[1, 0] * p[:, 0] + H[1, 1] * p[:, 1] + H[1, 2]) * w], axis=1)
