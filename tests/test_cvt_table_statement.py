"""CPU: properties of the restatement of the added colour conversions (tests/cvt_table_restate.py) that need no cv2."""
import numpy as np
import pytest

import cvt_table_restate as R


@pytest.fixture(scope="module")
def colours():
    return R.all_colours()


# Largest |channel difference| after forward then inverse over all 2^24 BGR colours, per channel (B, G, R), measured once from the
# restatement.  YCrCb never saturates, so only the two roundings remain; U and V saturate for strong blues / reds and
# greens (blue gives U = 239 but green gives V = -3.5 -> 0), which is where YUV loses up to 34 levels - in cv2 as well.
ROUND_TRIP = {"ycrcb": (1, 1, 1), "yuv": (1, 17, 34)}


@pytest.mark.parametrize("name", ["ycrcb", "yuv"])
def test_round_trip_bound_over_all_colours(colours, name):
    fwd, inv = {"ycrcb": (R.bgr2ycrcb, R.ycrcb2bgr), "yuv": (R.bgr2yuv, R.yuv2bgr)}[name]
    err = np.abs(inv(fwd(colours)).astype(np.int16) - colours)
    got = tuple(int(err[..., c].max()) for c in range(3))
    print(name, "round-trip maxima (B, G, R):", got)
    assert got == ROUND_TRIP[name]


def test_rgb_twin_is_the_bgr_code_on_the_reversed_image():
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (37, 41, 3), dtype=np.uint8)
    rev = np.ascontiguousarray(img[..., ::-1])
    for twin, base, side in (("RGB2YUV", "BGR2YUV", 0), ("RGB2XYZ", "BGR2XYZ", 0), ("YUV2RGB", "YUV2BGR", 1), ("YCRCB2RGB", "YCRCB2BGR", 1),
                             ("XYZ2RGB", "XYZ2BGR", 1), ("HLS2RGB", "HLS2BGR", 1)):
        exp = R.CODES[base](rev) if side == 0 else R.CODES[base](img)[..., ::-1]
        assert np.array_equal(R.CODES[twin](img), exp), twin
    assert np.array_equal(R.CODES["RGB2YCRCB"](img), R.bgr2ycrcb(rev))
    assert np.array_equal(R.CODES["RGB2GRAY"](img), R.bgr2gray(rev))
    assert np.array_equal(R.CODES["BGR2RGB"](img), rev)


def test_alpha_codes_are_plain_indexing():
    rng = np.random.default_rng(12)
    a = rng.integers(0, 256, (9, 13, 4), dtype=np.uint8)
    bgr = rng.integers(0, 256, (9, 13, 3), dtype=np.uint8)
    g = rng.integers(0, 256, (9, 13), dtype=np.uint8)
    assert np.array_equal(R.CODES["BGRA2BGR"](a), a[:, :, :3])
    assert np.array_equal(R.CODES["RGBA2BGR"](a), a[:, :, [2, 1, 0]])
    assert np.array_equal(R.CODES["BGRA2RGBA"](a), a[:, :, [2, 1, 0, 3]])
    out = R.CODES["BGR2BGRA"](bgr)
    assert out.shape == (9, 13, 4) and np.array_equal(out[:, :, :3], bgr) and (out[:, :, 3] == 255).all()
    out = R.CODES["BGR2RGBA"](bgr)
    assert np.array_equal(out[:, :, :3], bgr[:, :, ::-1]) and (out[:, :, 3] == 255).all()
    out = R.CODES["GRAY2BGRA"](g)
    assert all(np.array_equal(out[:, :, c], g) for c in range(3)) and (out[:, :, 3] == 255).all()
    assert np.array_equal(R.CODES["BGRA2GRAY"](a), R.bgr2gray(a[:, :, :3]))
    assert np.array_equal(R.CODES["RGBA2GRAY"](a), R.bgr2gray(a[:, :, [2, 1, 0]]))


def test_gray_to_bgra_and_back_is_the_identity():
    g = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(R.CODES["BGRA2GRAY"](R.CODES["GRAY2BGRA"](g)), g)       # 1868 + 9617 + 4899 = 2^14
    assert np.array_equal(R.CODES["RGBA2GRAY"](R.CODES["GRAY2BGRA"](g)), g)


KNOWN = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (128, 128, 128)]      # BGR: black, white, blue, green, red, mid-grey


def _round_sat(v):
    return int(min(255, max(0, np.floor(v + 0.5))))


def test_known_answers_from_the_analytic_matrices():
    """float64 from the analytic definitions (the difference channels on the integer Y, as OpenCV forms them), rounded and saturated."""
    for px in KNOWN:
        b, g, r = (float(v) for v in px)
        p = np.array([[px]], np.uint8)
        y = _round_sat(0.114 * b + 0.587 * g + 0.299 * r)
        assert R.bgr2yuv(p)[0, 0].tolist() == [y, _round_sat(0.492 * (b - y) + 128), _round_sat(0.877 * (r - y) + 128)], px
        assert R.bgr2ycrcb(p)[0, 0].tolist() == [y, _round_sat(0.713 * (r - y) + 128), _round_sat(0.564 * (b - y) + 128)], px
        xyz = [_round_sat(0.412453 * r + 0.357580 * g + 0.180423 * b), _round_sat(0.212671 * r + 0.715160 * g + 0.072169 * b),
               _round_sat(0.019334 * r + 0.119193 * g + 0.950227 * b)]
        assert R.bgr2xyz(p)[0, 0].tolist() == xyz, px
    # the literal values, so that a change of both sides at once is seen
    assert [R.bgr2yuv(np.array([[px]], np.uint8))[0, 0].tolist() for px in KNOWN] == \
        [[0, 128, 128], [255, 128, 128], [29, 239, 103], [150, 54, 0], [76, 91, 255], [128, 128, 128]]
    assert [R.bgr2xyz(np.array([[px]], np.uint8))[0, 0].tolist() for px in KNOWN] == \
        [[0, 0, 0], [242, 255, 255], [46, 18, 242], [91, 182, 30], [105, 54, 5], [122, 128, 139]]
    # the inverses: greys come back exactly through YUV and YCrCb; XYZ -> BGR is the analytic inverse matrix on the 8-bit (X, Y, Z)
    for px in ((0, 0, 0), (128, 128, 128)):
        p = np.array([[px]], np.uint8)
        assert R.yuv2bgr(R.bgr2yuv(p)).tolist() == p.tolist() and R.ycrcb2bgr(R.bgr2ycrcb(p)).tolist() == p.tolist()
    for px in KNOWN:
        x, y, z = (float(v) for v in R.bgr2xyz(np.array([[px]], np.uint8))[0, 0])
        exp = [_round_sat(0.055648 * x - 0.204043 * y + 1.057311 * z), _round_sat(-0.969256 * x + 1.875991 * y + 0.041556 * z),
               _round_sat(3.240479 * x - 1.53715 * y - 0.498535 * z)]
        assert R.xyz2bgr(np.array([[[x, y, z]]], np.uint8))[0, 0].tolist() == exp, px
    # HLS: (H, L, S) -> BGR.  L = 0 / 255 are black / white whatever the hue; S = 0 is the grey of L; full saturation at L = 128 gives
    # the primaries up to the rounding of 128 / 255 (p2 = 1.0, p1 = 2 * 0.50196 - 1 -> 1 level)
    hls = lambda h, l, s: R.hls2bgr(np.array([[[h, l, s]]], np.uint8))[0, 0].tolist()
    assert hls(77, 0, 200) == [0, 0, 0] and hls(77, 255, 200) == [255, 255, 255] and hls(33, 128, 0) == [128, 128, 128]
    assert hls(0, 128, 255) == [1, 1, 255] and hls(60, 128, 255) == [1, 255, 1] and hls(120, 128, 255) == [255, 1, 1]
    assert hls(30, 128, 255) == [1, 255, 255] and hls(180, 128, 255) == hls(0, 128, 255)
