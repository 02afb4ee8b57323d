"""CPU: the statement the Lab -> BGR kernels and the white balance are built on (tests/lab_inverse_restate.py), checked against
libvp's host tables, high-precision arithmetic, textbook CIE formulas, numpy and the reference's function bodies."""
import os
import sys
from fractions import Fraction

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lab_inverse_restate as R  # noqa: E402

mp.mp.prec = 200


def _ulp32(v):
    return float(np.spacing(np.float32(abs(float(v)))))


def _mp(v):
    return mp.mpf(v.numerator) / v.denominator if isinstance(v, Fraction) else mp.mpf(v)


def _tie(v):
    v = _mp(v)
    return abs(v - mp.floor(v) - mp.mpf(1) / 2)


def test_host_tables_equal_restatement():
    from vision import _vp
    yf, abxz, invg, C = _vp.get_lab_inv_tables()
    t = R.tables()
    assert np.array_equal(yf, t.yf)
    assert np.array_equal(abxz, t.abxz)
    assert np.array_equal(invg, t.invg)
    assert np.array_equal(C, t.C)
    assert C.tolist() == [[217, -836, 4715], [-3773, 7684, 185], [12615, -6296, -2223]]
    # the ranges color_lab.cpp's comments state
    assert t.yf[:, 0].min() == 0 and t.yf[:, 0].max() == R.BASE and t.yf[:, 1].min() == 2260 and t.yf[:, 1].max() == R.BASE
    assert t.abxz.min() == -1335 and t.abxz.max() == 88231


def test_index_ranges_cover_every_input():
    """ify + adiv and ify - bdiv stay inside abToXZ_b for every 8-bit (L, a, b); MIN_AB is the attained minimum."""
    t = R.tables()
    v = np.arange(256)
    adiv = ((5 * v * 53687 + (1 << 7)) >> 13) - R.ADIV_BIAS
    bdiv = ((v * 41943 + (1 << 4)) >> 9) - R.BDIV_BIAS
    ify = t.yf[:, 1]
    lo = min(ify.min() + adiv.min(), ify.min() - bdiv.max())
    hi = max(ify.max() + adiv.max(), ify.max() - bdiv.min())
    assert lo == R.MIN_AB and hi - R.MIN_AB < R.AB_TAB


def test_inverse_gamma_tie_margins():
    """Every sRGBInvGammaTab_b entry's exact argument 255 * sRGB(i / 4096) sits further from a rounding tie than the binary32 error
    of OpenCV's evaluation (binary64 pow rounded to binary32, times 255 in binary32: under 2 ulp32 of the argument), so no
    last-bit difference of pow can move an entry.  Minimum margin: 8.36e-5 at i = 3654 (242.49992)."""
    t = R.tables()
    worst = (1, None)
    for i in range(R.INV_GAMMA_TAB_SIZE):
        x = mp.mpf(i) / R.INV_GAMMA_TAB_SIZE
        g = x * mp.mpf(323) / 25 if x <= mp.mpf(7827) / 2500000 else x ** (mp.mpf(5) / 12) * mp.mpf(211) / 200 - mp.mpf(11) / 200
        exact = 255 * g
        m = _tie(exact)
        assert m > 2 * _ulp32(exact), i
        assert t.invg[i] == int(mp.nint(exact)), i
        worst = min(worst, (float(m), i), key=lambda p: p[0])
    assert worst[1] == 3654 and abs(worst[0] - 8.3645e-5) < 1e-8


def test_yf_and_coefficient_tie_margins():
    """LabToYF_b: the exact y and f(y) against the binary32 error of the four-operation recipe (3 roundings of values up to BASE: under
    2 ulp32).  One entry is closer than that - f(y) of L = 246, 15885.50101, 1.04 ulp32 from the tie - so its value is decided by the
    binary32 statement sequence, which the restatement follows operation by operation; it agrees with the exact rounding.  Every other
    entry: minimum margin recorded below.  Matrix: exact decimal products against binary64 error (margin 0.0956)."""
    t = R.tables()
    close, worst = [], (1, None)
    for L in range(256):
        Ls = Fraction(L * 100, 255)
        if L <= R.L_LINEAR_MAX:
            y = R.BASE * Ls * Fraction(27, 24389)
            fy = Fraction(16, 116) + Ls * Fraction(27, 24389) * Fraction(841, 108)
        else:
            fy = (Ls + 16) / 116
            y = R.BASE * fy ** 3
        for col, v in ((0, y), (1, R.BASE * fy)):
            m = _tie(v)
            assert t.yf[L, col] == int(mp.nint(_mp(v))), (L, col)
            if m <= 2 * _ulp32(v):
                close.append((L, col))
            else:
                worst = min(worst, (float(m), (L, col)), key=lambda p: p[0])
    assert close == [(246, 1)]
    assert worst[0] > 0.0015
    dec = [["0.055648", "-0.204043", "1.057311"], ["-0.969256", "1.875991", "0.041556"], ["3.240479", "-1.53715", "-0.498535"]]
    white = ["0.950456", "1", "1.088754"]
    cm = min(float(_tie(4096 * Fraction(dec[c][j]) * Fraction(white[j]))) for c in range(3) for j in range(3))
    assert cm > 0.09 and cm > 1e3 * np.spacing(13000.0)


def test_known_answers():
    lab = np.array([[[0, 128, 128], [255, 128, 128]]], np.uint8)
    assert R.lab2bgr(lab).tolist() == [[[0, 0, 0], [255, 255, 255]]]


def test_restatement_against_textbook_on_all_inputs():
    """All 2^24 inputs against float64 CIE formulas.  Bound, derived: the output is a table look-up g(v) of the Q12 index v, where
    255 g has slope at most 12.92 * 255 / 4096 = 0.8043 per index step (the linear segment; the power segment is flatter past the
    threshold), and each entry is within 0.5 of 255 g at its index.  The index differs from 4096 * the exact linear value by the
    fixed-point error of x, y, z and the Q12 coefficients (measured below, E), the descale rounding (0.5) and the clamp to 4095
    (1).  So |out - textbook| <= 0.5 + 0.8043 (E + 1.5).  Observed maximum: 2.615 at (L, a, b) = (254, 155, 16)."""
    t = R.tables()
    ab = np.stack(np.meshgrid(np.arange(256), np.arange(256), indexing="ij"), -1).reshape(-1, 2)
    rows = (R.XYZ2SRGB[2], R.XYZ2SRGB[1], R.XYZ2SRGB[0])
    dev, E = 0.0, 0.0
    for L in range(256):
        lab = np.concatenate([np.full((65536, 1), L), ab], 1).astype(np.uint8)
        dev = max(dev, float(np.abs(R.lab2bgr(lab).astype(np.float64) - R.textbook_lab2bgr(lab)).max()))
        # fixed-point linear value (before the descale) against the exact one, both clamped to the table's domain
        Li, a, b = (lab[:, c].astype(np.int64) for c in range(3))
        y, ify = t.yf[Li, 0], t.yf[Li, 1]
        x = t.abxz[ify + ((5 * a * 53687 + 128) >> 13) - R.ADIV_BIAS - R.MIN_AB]
        z = t.abxz[ify - (((b * 41943 + 16) >> 9) - R.BDIV_BIAS) - R.MIN_AB]
        fy = (Li * (100.0 / 255.0) + 16.0) / 116.0
        d = 6.0 / 29.0

        def finv(v):
            return np.where(v > d, v ** 3, 3 * d * d * (v - 4.0 / 29.0))
        X, Y, Z = R.WHITE[0] * finv(fy + (a - 128) / 500.0), finv(fy), R.WHITE[2] * finv(fy - (b - 128) / 200.0)
        for c in range(3):
            fixed = (t.C[c, 0] * x + t.C[c, 1] * y + t.C[c, 2] * z) / float(1 << 14)
            exact = 4096.0 * (rows[c][0] * X + rows[c][1] * Y + rows[c][2] * Z)
            E = max(E, float(np.abs(np.clip(fixed, 0, 4096) - np.clip(exact, 0, 4096)).max()))
    bound = 0.5 + 12.92 * 255 / 4096 * (E + 1.5)
    assert dev <= bound, (dev, E, bound)
    assert abs(dev - 2.615) < 1e-3, dev


def test_chunked_mean_equals_numpy():
    rng = np.random.default_rng(1)
    for h, w in [(1, 1), (1, 8191), (1, 8193), (3, 5), (97, 211), (720, 1280), (1080, 1920), (1081, 1917), (2160, 3840), (2161, 4099)]:
        for plane in (rng.integers(0, 256, (h, w), dtype=np.uint8), np.full((h, w), 200, np.uint8),
                      rng.integers(100, 140, (h, w), dtype=np.uint8)):
            assert R.chunked_mean(plane) == np.mean(plane.astype(np.float32)), (h, w)
            assert R.chunked_mean(plane).dtype == np.float32


def test_wrap_equals_astype():
    rng = np.random.default_rng(2)
    v = rng.uniform(-130, 390, 2_000_000).astype(np.float32)
    v[:6] = [-1.5, 256.2, 300.9, -0.5, 255.99, 0.0]
    assert np.array_equal(R.wrap_u8(v), v.astype(np.uint8))
    assert R.wrap_u8(np.float32([-1.5, 256.2, 300.9])).tolist() == [255, 0, 44]


def _lab(oracle, bgr):
    return oracle.bgr2lab(bgr)


def _reference_white_balance(lab_u8):
    """utils/color.py:370-378, cv2 replaced by the restatement (cvtColor LAB2BGR) and numpy (split / merge)."""
    lab_img = lab_u8.astype(np.float32)
    lab_l, lab_a, lab_b = (np.ascontiguousarray(lab_img[:, :, c]) for c in range(3))
    a_avg = np.mean(lab_a)
    b_avg = np.mean(lab_b)
    lab_a -= a_avg - 128
    lab_b -= b_avg - 128
    lab_img = np.dstack((lab_l, lab_a, lab_b))
    return R.lab2bgr(lab_img.astype(np.uint8))


def _reference_white_balance_blur(lab_u8, kernel_size):
    """utils/color.py:381-392, cv2.blur replaced by the restated box mean."""
    kernel_size //= 2
    kernel_size = 2 * kernel_size + 1
    lab_img = lab_u8.astype(np.float32)
    lab_l, lab_a, lab_b = (np.ascontiguousarray(lab_img[:, :, c]) for c in range(3))
    lab_a_avg = R.box_mean(lab_a.astype(np.uint8), kernel_size)
    lab_b_avg = R.box_mean(lab_b.astype(np.uint8), kernel_size)
    lab_a -= lab_a_avg - 128
    lab_b -= lab_b_avg - 128
    lab_img = np.dstack((lab_l, lab_a, lab_b))
    return R.lab2bgr(lab_img.astype(np.uint8))


def test_box_mean_against_direct_sum():
    rng = np.random.default_rng(3)
    p = rng.integers(0, 256, (9, 14), dtype=np.uint8)
    for k in (1, 3, 5, 31):
        r = k // 2
        ext = np.pad(p.astype(np.int64), r, mode="edge")
        direct = np.array([[ext[y:y + k, x:x + k].sum() for x in range(14)] for y in range(9)], np.float64)
        assert np.array_equal(R.box_mean(p, k), (direct * (1.0 / (k * k))).astype(np.float32))


def test_restated_white_balance_equals_reference_bodies(oracle):
    rng = np.random.default_rng(4)
    for h, w in [(1, 1), (5, 7), (64, 48), (121, 203)]:
        bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        bgr[..., 2] //= 2                       # a colour cast, so that the shifts are not near zero
        lab = _lab(oracle, bgr)
        got, means = R.white_balance_bgr(lab)
        assert np.array_equal(got, _reference_white_balance(lab))
        assert means == (np.mean(lab[..., 1].astype(np.float32)), np.mean(lab[..., 2].astype(np.float32)))
        for ks in (1, 2, 3, 5, 31, 255):
            assert np.array_equal(R.white_balance_bgr_blur(lab, ks), _reference_white_balance_blur(lab, ks)), (h, w, ks)
    with pytest.raises(ValueError):
        R.white_balance_bgr_blur(lab, -1)


def test_new_names_are_bound():
    """lab_to_bgr and the two white-balance names are no longer placeholders: without a GPU they fail as every libvp operator does
    (VpError), with one they return an image."""
    import torch
    from vision import _vp
    from vision.utils import color
    img = np.zeros((4, 4, 3), np.uint8)
    calls = (lambda m: color.lab_to_bgr(m)[0], color.white_balance_bgr, lambda m: color.white_balance_bgr_blur(m, 3))
    for f in calls:
        if torch.cuda.is_available():
            assert f(img).shape == (4, 4, 3)
        else:
            with pytest.raises(_vp.VpError):
                f(img)
    from vision import cv2_facade
    with pytest.raises(cv2_facade.error):                    # what the reference's cv2.blur raises
        color.white_balance_bgr_blur(img, -1)
    assert _vp.lib().vp_white_balance_u8(None, _vp.ptr(img), 12, 4, 4, 0, _vp.ptr(img), None) == -1
