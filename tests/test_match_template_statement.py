"""CPU suite that pins tests/match_template_restate.py, the statement of cv2.matchTemplate the GPU suite compares with: every score is
worked out a second time here, pixel by pixel, from Python integers and math.sqrt in the order DESIGN.md section 4.27 gives, and the
two inputs that reach every rule of the normed methods are checked rule by rule.  No library code runs."""
import math
import struct

import numpy as np
import pytest

import match_template_restate as R

F32 = lambda v: struct.unpack("f", struct.pack("f", v))[0]
EPS10 = 10 * 2.0 ** -23


def _by_hand(image, templ, method, x, y):
    """one score from Python integers; also the rule that gave it (None for the unnormed methods)"""
    I = image if image.ndim == 3 else image[:, :, None]
    T = templ if templ.ndim == 3 else templ[:, :, None]
    th, tw, cn = T.shape
    n = tw * th
    win = [[[int(I[y + j, x + i, c]) for c in range(cn)] for i in range(tw)] for j in range(th)]
    tt = [[[int(T[j, i, c]) for c in range(cn)] for i in range(tw)] for j in range(th)]
    cells = [(j, i, c) for j in range(th) for i in range(tw) for c in range(cn)]
    C = sum(win[j][i][c] * tt[j][i][c] for j, i, c in cells)
    S2 = sum(win[j][i][c] ** 2 for j, i, c in cells)
    T2 = sum(tt[j][i][c] ** 2 for j, i, c in cells)
    S1 = [sum(win[j][i][c] for j in range(th) for i in range(tw)) for c in range(cn)]
    T1 = [sum(tt[j][i][c] for j in range(th) for i in range(tw)) for c in range(cn)]
    d_int = n * S2
    if method in (R.CCORR, R.CCORR_NORMED):
        num = float(C)
    elif method in (R.SQDIFF, R.SQDIFF_NORMED):
        num = float(S2 - 2 * C + T2)
    else:
        num = float(n * C - sum(a * b for a, b in zip(S1, T1))) / float(n)
        d_int -= sum(a * a for a in S1)
    if method not in R.NORMED:
        return F32(num), None
    tn_int = n * T2 - (sum(a * a for a in T1) if method == R.CCOEFF_NORMED else 0)
    if method == R.CCOEFF_NORMED and tn_int == 0:
        return 1.0, "constant"
    templ_norm = math.sqrt(float(tn_int) / float(n))
    diff2 = float(d_int) / float(n)
    t = 0.0 if diff2 <= min(0.5, EPS10 * float(S2)) else math.sqrt(diff2) * templ_norm
    if abs(num) < t:
        return F32(num / t), 1
    if abs(num) < t * 1.125:
        return (1.0 if num > 0 else -1.0), 2
    return (1.0 if method == R.SQDIFF_NORMED else 0.0), (0 if t == 0.0 else 3)


def _check_all(image, templ):
    """the statement against the scalar arithmetic at every pixel and method; -> {method: set of rules met}"""
    rules = {}
    for method in R.METHODS:
        got = R.match_template(image, templ, method)
        rh, rw = image.shape[0] - templ.shape[0] + 1, image.shape[1] - templ.shape[1] + 1
        assert got.dtype == np.float32 and got.shape == (rh, rw)
        met = set()
        for y in range(rh):
            for x in range(rw):
                want, rule = _by_hand(image, templ, method, x, y)
                assert struct.pack("f", got[y, x]) == struct.pack("f", want), (method, x, y, got[y, x], want)
                met.add(rule)
        if method in R.NORMED and "constant" not in met:
            b = R.branches(image, templ, method)
            assert set(np.unique(b).tolist()) == met, (method, met)
        rules[method] = met
    return rules


def branch_image():
    """12 x 13 random grey, a constant 4 x 5 patch of 7 at the top left, a zero 4 x 5 patch at the bottom right"""
    img = np.random.default_rng(20).integers(0, 256, (12, 13), dtype=np.uint8)
    img[:4, :5] = 7
    img[-4:, -5:] = 0
    return img


def far_pair():
    """a 6 x 6 image of 2s against a 3 x 3 template of 200s, one pixel changed in each: SQDIFF_NORMED beyond 1.125 t at every pixel"""
    img = np.full((6, 6), 2, np.uint8)
    img[2, 3] = 3
    templ = np.full((3, 3), 200, np.uint8)
    templ[1, 1] = 201
    return img, templ


def test_every_rule_of_the_normed_methods_is_reached():
    img = branch_image()
    templ = img[3:7, 4:9].copy()
    assert templ.shape == (4, 5) and len(np.unique(templ)) > 1
    rules = _check_all(img, templ)
    assert rules[R.SQDIFF_NORMED] >= {0, 1, 3} and rules[R.CCORR_NORMED] >= {0, 1} and rules[R.CCOEFF_NORMED] >= {0, 1}
    assert 2 in rules[R.SQDIFF_NORMED] | rules[R.CCORR_NORMED] | rules[R.CCOEFF_NORMED], "the clamp to +-1 is not reached"
    # t = 0: the zero window gives 0, or 1 for SQDIFF_NORMED; the constant window has no variance left for CCOEFF_NORMED
    assert R.match_template(img, templ, R.CCORR_NORMED)[-1, -1] == 0.0 and R.match_template(img, templ, R.SQDIFF_NORMED)[-1, -1] == 1.0
    assert R.match_template(img, templ, R.CCOEFF_NORMED)[0, 0] == 0.0 and R.branches(img, templ, R.CCOEFF_NORMED)[0, 0] == 0
    # the perfect match: SQDIFF is 0 there and nowhere else is CCOEFF_NORMED larger
    assert R.match_template(img, templ, R.SQDIFF)[3, 4] == 0.0 and R.match_template(img, templ, R.SQDIFF_NORMED)[3, 4] == 0.0
    assert R.best_match(img, templ, R.CCOEFF_NORMED)[0] == (4, 3) and R.best_match(img, templ, R.SQDIFF)[0] == (4, 3)
    assert abs(R.match_template(img, templ, R.CCOEFF_NORMED)[3, 4] - 1.0) <= 2.0 ** -23
    # a template that is constant per channel: CCOEFF_NORMED is 1 everywhere
    flat = np.full((4, 5), 7, np.uint8)
    assert _check_all(img, flat)[R.CCOEFF_NORMED] == {"constant"}
    assert (R.match_template(img, flat, R.CCOEFF_NORMED) == 1.0).all()


def test_sqdiff_normed_beyond_the_clamp_everywhere():
    img, templ = far_pair()
    rules = _check_all(img, templ)
    assert rules[R.SQDIFF_NORMED] == {3}
    assert (R.match_template(img, templ, R.SQDIFF_NORMED) == 1.0).all()
    # one window by hand: eight 2s and one 3 against eight 200s and one 201 at the centre
    # S2 = 8 * 4 + 9 = 41, T2 = 8 * 40000 + 40401 = 360401, C at (2, 1) [the 3 under the 201] = 8 * 400 + 603 = 3803
    assert R.sums(img, templ)[0][1, 2] == 3803 and R.sums(img, templ)[1][1, 2] == 41 and R.sums(img, templ)[3] == 360401
    assert R.match_template(img, templ, R.SQDIFF)[1, 2] == 41 - 2 * 3803 + 360401


def test_one_by_one_template():
    img = np.array([[0, 1, 2], [3, 200, 255]], np.uint8)
    templ = np.array([[3]], np.uint8)
    _check_all(img, templ)
    assert R.match_template(img, templ, R.CCORR).tolist() == [[0.0, 3.0, 6.0], [9.0, 600.0, 765.0]]
    assert R.match_template(img, templ, R.SQDIFF).tolist() == [[9.0, 4.0, 1.0], [0.0, 197.0 ** 2, 252.0 ** 2]]
    assert (R.match_template(img, templ, R.CCOEFF) == 0.0).all()          # a single pixel has no deviation from its mean
    assert (R.match_template(img, templ, R.CCOEFF_NORMED) == 1.0).all()   # ... and the template is constant
    # CCORR_NORMED: I T / sqrt(I^2 T^2) = 1 wherever I > 0 (division or clamp), 0 at the zero pixel (t = 0)
    assert R.match_template(img, templ, R.CCORR_NORMED)[0, 0] == 0.0
    assert np.abs(R.match_template(img, templ, R.CCORR_NORMED).ravel()[1:] - 1.0).max() <= 2.0 ** -23


def test_template_equal_to_the_image():
    img = np.random.default_rng(3).integers(0, 256, (7, 9), dtype=np.uint8)
    _check_all(img, img.copy())
    s = int((img.astype(np.int64) ** 2).sum())
    assert R.match_template(img, img, R.CCORR).shape == (1, 1) and R.match_template(img, img, R.CCORR)[0, 0] == np.float32(s)
    assert R.match_template(img, img, R.SQDIFF)[0, 0] == 0.0 and R.match_template(img, img, R.SQDIFF_NORMED)[0, 0] == 0.0
    for m in (R.CCORR_NORMED, R.CCOEFF_NORMED):
        assert abs(R.match_template(img, img, m)[0, 0] - 1.0) <= 2.0 ** -23


def test_three_channels_with_the_sums_written_out():
    # image 2 x 3, template 2 x 2, channels (b, g, r)
    img = np.array([[[1, 2, 3], [4, 5, 6], [7, 8, 9]], [[10, 11, 12], [13, 14, 15], [16, 17, 18]]], np.uint8)
    templ = np.array([[[1, 0, 2], [0, 3, 0]], [[2, 0, 0], [0, 0, 1]]], np.uint8)
    C, S2, S1, T2, T1, N = R.sums(img, templ)
    # window x = 0: (1,2,3) (4,5,6) / (10,11,12) (13,14,15);  x = 1: (4,5,6) (7,8,9) / (13,14,15) (16,17,18)
    assert C.tolist() == [[1 * 1 + 3 * 2 + 5 * 3 + 10 * 2 + 15 * 1, 4 * 1 + 6 * 2 + 8 * 3 + 13 * 2 + 18 * 1]] == [[57, 84]]
    assert S2.tolist() == [[1 + 4 + 9 + 16 + 25 + 36 + 100 + 121 + 144 + 169 + 196 + 225, 16 + 25 + 36 + 49 + 64 + 81 + 169 + 196 + 225 + 256 + 289 + 324]]
    assert S1.tolist() == [[[1 + 4 + 10 + 13, 4 + 7 + 13 + 16]], [[2 + 5 + 11 + 14, 5 + 8 + 14 + 17]], [[3 + 6 + 12 + 15, 6 + 9 + 15 + 18]]]
    assert (T2, T1.tolist(), N) == (1 + 4 + 9 + 4 + 1, [3, 3, 3], 4)
    # CCOEFF at x = 0: (4 * 57 - (28 * 3 + 32 * 3 + 36 * 3)) / 4 = (228 - 288) / 4 = -15
    assert R.match_template(img, templ, R.CCOEFF).tolist() == [[-15.0, (4 * 84 - (40 + 44 + 48) * 3) / 4]]
    assert R.match_template(img, templ, R.SQDIFF).tolist() == [[1046.0 - 114 + 19, 1730.0 - 168 + 19]]
    _check_all(img, templ)


@pytest.mark.parametrize("cn", (1, 2, 3, 4))
def test_random_images_of_every_channel_count(cn):
    rng = np.random.default_rng(cn)
    img = rng.integers(0, 256, (6, 8, cn), dtype=np.uint8)
    img[:3, :3] = 0
    _check_all(img if cn > 1 else img[:, :, 0], (img[2:5, 3:6] if cn > 1 else img[2:5, 3:6, 0]).copy())


def test_the_bounds_of_the_size_limit():
    # N cn = 65536 bytes of 255 against 255: the largest sums there are
    c = 255 * 255 * 65536
    assert c == 4261478400 and 2 ** 31 < c < 2 ** 32 and 65536 * c < 2 ** 48
    img, templ = np.full((5, 4), 255, np.uint8), np.full((4, 4), 255, np.uint8)
    assert R.match_template(img, templ, R.CCORR).tolist() == [[16 * 65025.0]] * 2
    assert R.match_template(img, templ, R.SQDIFF).tolist() == [[0.0]] * 2 and R.match_template(img, templ, R.CCOEFF_NORMED).tolist() == [[1.0]] * 2
