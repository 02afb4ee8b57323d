"""cv2.cornerMinEigenVal, cv2.cornerHarris and cv2.goodFeaturesToTrack as this project defines them, restated
in numpy and plain Python from the contract and from OpenCV's published algorithm (imgproc/src/corner.cpp cornerEigenValsVecs,
featureselect.cpp goodFeaturesToTrack).  Independent of the library: integer Sobel by slicing, int64 box sums, numpy float64 for the
eigenvalue formula in the contract's operation order, plain Python for the selection.

The response is NOT cv2's float32 arithmetic: it is the exact value of what that arithmetic approximates, rounded to float32 once."""
import numpy as np

CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101 = 0, 1, 2, 3, 4
BORDERS = (REFLECT_101, REPLICATE, REFLECT, CONSTANT)
MAX_BLOCK = 31
MAX_DERIV = 1020


def border_index(p, n, border):
    """cv::borderInterpolate: the index in [0, n) coordinate p reads, -1 for the constant border"""
    if 0 <= p < n:
        return p
    if border == REPLICATE:
        return 0 if p < 0 else n - 1
    if border == CONSTANT:
        return -1
    if border not in (REFLECT, REFLECT_101):
        raise ValueError("unsupported border")
    if n == 1:
        return 0
    delta = 1 if border == REFLECT_101 else 0
    while not 0 <= p < n:
        p = -p - 1 + delta if p < 0 else n - 1 - (p - n) - delta
    return p


def extend(img, top, bottom, left, right, border):
    """cv::copyMakeBorder of a 2-D integer array (constant value 0), as int64"""
    h, w = img.shape
    ys = [border_index(y, h, border) for y in range(-top, h + bottom)]
    xs = [border_index(x, w, border) for x in range(-left, w + right)]
    src = np.zeros((h + 1, w + 1), np.int64)           # row / column -1 reads the zero pad
    src[:h, :w] = img
    return src[np.array(ys)][:, np.array(xs)]


def sobel_pair(img, border):
    """(Dx, Dy): the integer 3x3 Sobel derivatives of a uint8 image, int64 (h, w)"""
    h, w = img.shape
    e = extend(np.asarray(img, np.int64), 1, 1, 1, 1, border)
    s = lambda dy, dx: e[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    dx = (s(-1, 1) + 2 * s(0, 1) + s(1, 1)) - (s(-1, -1) + 2 * s(0, -1) + s(1, -1))
    dy = (s(1, -1) + 2 * s(1, 0) + s(1, 1)) - (s(-1, -1) + 2 * s(-1, 0) + s(-1, 1))
    return dx, dy


def box_sum(p, block, border):
    """unnormalised block x block box sum of an integer image, anchor block // 2, the border applied to THIS image (cv::boxFilter)"""
    h, w = p.shape
    a = block // 2
    e = extend(p, a, block - 1 - a, a, block - 1 - a, border)
    out = np.zeros((h, w), np.int64)
    for dy in range(block):
        for dx in range(block):
            out += e[dy:dy + h, dx:dx + w]
    return out


def structure_tensor(img, block, border=REFLECT_101):
    """(Sxx, Sxy, Syy) int64"""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 2 or img.size == 0:
        raise ValueError("expected a non-empty uint8 (h, w) image")
    if not 1 <= block <= MAX_BLOCK:
        raise ValueError("blockSize outside 1..31")
    dx, dy = sobel_pair(img, border)
    return box_sum(dx * dx, block, border), box_sum(dx * dy, block, border), box_sum(dy * dy, block, border)


def scale(block):
    return 1.0 / (4.0 * block * 255.0)


def min_eigen_val(img, block=3, border=REFLECT_101):
    sxx, sxy, syy = structure_tensor(img, block, border)
    s = np.float64(scale(block))
    a = sxx.astype(np.float64) * 0.5
    b = sxy.astype(np.float64)
    c = syy.astype(np.float64) * 0.5
    lam = (a + c) - np.sqrt((a - c) * (a - c) + b * b)
    return (lam * (s * s)).astype(np.float32)


def harris(img, block, k=0.04, border=REFLECT_101):
    sxx, sxy, syy = structure_tensor(img, block, border)
    s = np.float64(scale(block))
    a = sxx.astype(np.float64)
    b = sxy.astype(np.float64)
    c = syy.astype(np.float64)
    hh = (a * c - b * b) - np.float64(k) * ((a + c) * (a + c))
    return (hh * ((s * s) * (s * s))).astype(np.float32)


def threshold_of(resp, quality, mask=None):
    """(maxVal, t) or (None, None) when the mask admits no pixel"""
    vals = resp if mask is None else resp[np.asarray(mask) != 0]
    if vals.size == 0:
        return None, None
    mx = np.float32(vals.max())
    return mx, np.float32(np.float64(mx) * np.float64(quality))


def candidates(resp, t, mask=None):
    """selection step 3, the contract's wording: [(resp, y, x)] in raster order"""
    h, w = resp.shape
    out = []
    for y in range(1, h - 1):
        for x in range(1, w - 1):
            v = resp[y, x]
            if not (v > t and v != 0) or (mask is not None and mask[y, x] == 0):
                continue
            nb = resp[y - 1:y + 2, x - 1:x + 2]
            if all(v >= n for n in nb.ravel() if n > t):
                out.append((v, y, x))
    return out


def candidates_cv2(resp, t, mask=None):
    """the same step as featureselect.cpp words it: threshold(eig, eig, t, 0, THRESH_TOZERO); dilate(eig, tmp, 3x3); val != 0 and
    val == tmp[y, x].  cv::dilate's border never wins: the maximum runs over the neighbours inside the image."""
    h, w = resp.shape
    z = np.where(resp > t, resp, np.float32(0)).astype(np.float32)
    out = []
    for y in range(1, h - 1):
        for x in range(1, w - 1):
            v = z[y, x]
            if v != 0 and v == z[y - 1:y + 2, x - 1:x + 2].max() and (mask is None or mask[y, x] != 0):
                out.append((v, y, x))
    return out


def select(cands, w, max_corners, min_distance):
    """steps 4 and 5: order by response descending, equal responses by larger raster index first; greedy minDistance; [(x, y)]"""
    order = sorted(cands, key=lambda c: (-float(c[0]), -(c[1] * w + c[2])))
    md2 = float(min_distance) * float(min_distance)
    kept = []
    for _, y, x in order:
        if min_distance >= 1 and any((x - kx) * (x - kx) + (y - ky) * (y - ky) < md2 for kx, ky in kept):
            continue
        kept.append((x, y))
        if max_corners > 0 and len(kept) == max_corners:
            break
    return kept


def good_features(img, max_corners, quality=0.01, min_distance=10, mask=None, block=3, use_harris=False, k=0.04):
    """float32 (N, 1, 2) of (x, y), or None"""
    img = np.asarray(img)
    h, w = img.shape
    if h < 3 or w < 3:
        return None
    resp = harris(img, block, k) if use_harris else min_eigen_val(img, block)
    if mask is not None:
        mask = np.asarray(mask)
        if mask.shape != img.shape:
            raise ValueError("the mask must have the size of the image")
    _, t = threshold_of(resp, quality, mask)
    if t is None:
        return None
    kept = select(candidates(resp, t, mask), w, max_corners, min_distance)
    if not kept:
        return None
    return np.array(kept, np.float32).reshape(-1, 1, 2)
