"""Live comparison of tests/corners_restate.py with a real OpenCV's cornerMinEigenVal, cornerHarris and goodFeaturesToTrack.  Skipped
where `cv2` is not importable.  CPU-only.  The contract is not cv2's float32 arithmetic but the exact value of
what it approximates, so the maps are compared within a bound and the corner sets outside the band that bound leaves open.

The bound, on paper.  cv2 scales Dx and Dy by s in float32 (one rounding each, relative 2^-24 = e), multiplies (one more), and adds the
n = blockSize^2 products of a window in float32 in some order: the sum of n terms carries at most (n - 1) e times the sum of their
magnitudes, so each of Sxx s^2, Syy s^2 is off by at most (n + 2) e times itself (to first order) and Sxy s^2 by at most (n + 2) e
sum |Dx Dy| s^2 <= (n + 2) e (Sxx + Syy) s^2 / 2.  L = (a + c) - sqrt((a - c)^2 + b^2) moves by at most |da| + |dc| + |db| (its partial
derivatives are at most 1 in magnitude), and its own five float32 operations add at most 5 e (a + c) more.  With a = Sxx s^2 / 2,
b = Sxy s^2, c = Syy s^2 / 2 that is (n + 2) e (Sxx + Syy) s^2 + 5 e (Sxx + Syy) s^2 / 2; the test allows
E = 2 (n + 8) e (Sxx + Syy) s^2, twice the first-order figure.  The Harris response is a product of two such sums: its bound is
E_H = 4 (n + 8) e (1 + 4 |k|) ((Sxx + Syy) s^2)^2."""
import numpy as np
import pytest

import corners_restate as R

cv2 = pytest.importorskip("cv2")
if not hasattr(cv2, "connectedComponentsWithStats") or getattr(cv2, "__name__", "") != "cv2" or "vision" in getattr(cv2, "__file__", ""):
    pytest.skip("the cv2 facade of this repo is not a reference", allow_module_level=True)

EPS = 2.0 ** -24


def _images():
    rng = np.random.default_rng(31)
    yield "grey", rng.integers(0, 256, (67, 35), dtype=np.uint8)
    yy, xx = np.indices((48, 80))
    yield "checker", (((yy // 8 + xx // 8) % 2) * 255).astype(np.uint8)
    rects = np.zeros((60, 90), np.uint8)
    rects[10:30, 15:50] = 255
    rects[35:55, 40:80] = 128
    yield "rects", rects
    yield "smooth", (127 + 100 * np.sin(xx / 7.0) * np.cos(yy / 5.0)).astype(np.uint8)


def _bound(img, block, k=None):
    sxx, _, syy = R.structure_tensor(img, block)
    s = R.scale(block)
    tr = (sxx + syy).astype(np.float64) * (s * s)
    n = block * block
    if k is None:
        return 2 * (n + 8) * EPS * tr
    return 4 * (n + 8) * EPS * (1 + 4 * abs(k)) * tr * tr


@pytest.mark.parametrize("block", (1, 2, 3, 5, 7, 15))
def test_response_maps_are_within_the_float32_bound_of_cv2(block):
    for name, img in _images():
        ours = R.min_eigen_val(img, block).astype(np.float64)
        theirs = cv2.cornerMinEigenVal(img, block, ksize=3).astype(np.float64)
        diff, bound = np.abs(ours - theirs), _bound(img, block)
        print(name, block, "min eigenvalue: largest difference", diff.max(), "largest bound", bound.max())
        assert (diff <= bound + 1e-12).all(), (name, block, float((diff - bound).max()))
        for k in (0.04, 0.2):
            ours = R.harris(img, block, k).astype(np.float64)
            theirs = cv2.cornerHarris(img, block, 3, k).astype(np.float64)
            diff, bound = np.abs(ours - theirs), _bound(img, block, k)
            print(name, block, k, "Harris: largest difference", diff.max(), "largest bound", bound.max())
            assert (diff <= bound + 1e-12).all(), (name, block, k, float((diff - bound).max()))


@pytest.mark.parametrize("block", (2, 3, 7))
def test_corner_sets_agree_outside_the_band_the_bound_leaves_open(block):
    """all corners, no distance: the order does not enter.  A candidate is certain when its response clears the threshold and every
    neighbour above the threshold by more than the two bounds involved; it is possible when it misses neither by more than them.  cv2
    must return every certain one and nothing that is not possible."""
    for name, img in _images():
        resp = R.min_eigen_val(img, block).astype(np.float64)
        e = _bound(img, block)
        h, w = resp.shape
        for quality in (0.01, 0.3):
            t = float(resp.max()) * quality
            et = float(e.max()) * quality + EPS * abs(t)
            certain, possible = set(), set()
            for y in range(1, h - 1):
                for x in range(1, w - 1):
                    v, ev = resp[y, x], e[y, x]
                    nb, en = resp[y - 1:y + 2, x - 1:x + 2], e[y - 1:y + 2, x - 1:x + 2]
                    if v + ev > t - et and v + ev > 0 and (v + ev >= nb - en).all():
                        possible.add((x, y))
                    others = np.ones((3, 3), bool)
                    others[1, 1] = False
                    if v - ev > t + et and v - ev > 0 and (v - ev > nb + en)[others].all():
                        certain.add((x, y))
            got = cv2.goodFeaturesToTrack(img, 0, quality, 0, blockSize=block)
            got = set() if got is None else {(int(px), int(py)) for px, py in got.reshape(-1, 2)}
            print(name, block, quality, "cv2", len(got), "certain", len(certain), "possible", len(possible))
            assert certain <= got <= possible, (name, block, quality, sorted(certain - got), sorted(got - possible))
