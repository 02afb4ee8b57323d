"""GPU: the colour conversions beside the first eight codes (YUV, XYZ, the inverses, RGB order, alpha and reorders), bit-equal to the
restatement (tests/cvt_table_restate.py; the RGB twins of the first eight codes against the oracle / the Lab inverse restatement of
the BGR code on the channel-reversed image), in both kernel forms, for host images and device images."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvt_table_restate as R  # noqa: E402
import lab_inverse_restate as LR  # noqa: E402

pytestmark = pytest.mark.gpu

ALL_CODES = sorted(set(R.CODES) | set(R.EXISTING_TWINS))
THREE_CHANNEL_SOURCE = [c for c in ALL_CODES if R.SOURCE_CHANNELS.get(c, 3) == 3]
ALPHA = ["BGRA2BGR", "RGBA2BGR", "BGR2BGRA", "BGR2RGBA", "BGRA2RGBA", "GRAY2BGRA", "BGRA2GRAY", "RGBA2GRAY"]


def _expect(oracle, name, img):
    """the restatement of code `name` on `img` (any row pitch)"""
    img = np.ascontiguousarray(img)
    if name in R.CODES:
        return R.CODES[name](img)
    base, side = R.EXISTING_TWINS[name]
    fn = LR.lab2bgr if base == "lab2bgr" else getattr(oracle, base)
    if side == "source":
        return fn(R.swap_rb(img))
    return R.swap_rb(fn(img))


def _channels(vp, name):
    return vp.CVT_CHANNELS.get(getattr(vp, name), (3, 3))


@pytest.fixture(params=[1, 0], ids=["flat", "generic"])
def flat(request, vp):
    ctx = vp.default_context()
    ctx.set_option(vp.OPT_FLAT_OPS, request.param)
    yield request.param
    ctx.set_option(vp.OPT_FLAT_OPS, 1)


@pytest.fixture(scope="module")
def colours():
    return R.all_colours()


def _cvt_u8(vp, name, src, want_dst=True, planes_mask=0):
    """vp_cvt_color_u8 on a host image (its row pitch passed on): (interleaved result or None, [planes])"""
    scn, dcn = _channels(vp, name)
    h, w = src.shape[:2]
    dst = np.zeros((h, w) if dcn == 1 else (h, w, dcn), np.uint8) if want_dst else None
    planes = [np.zeros((h, w), np.uint8) if planes_mask & (1 << c) else None for c in range(3)]
    arr = (vp.C.c_void_p * 3)(*[vp.ptr(p) for p in planes])
    ctx = vp.default_context()
    vp.check(vp.lib().vp_cvt_color_u8(ctx.handle, getattr(vp, name), vp.ptr(src), src.strides[0], w, h, vp.ptr(dst), arr if planes_mask else None), ctx.handle)
    return dst, planes


def _cvt_dev(vp, name, ptr, stride, w, h):
    """vp_cvt_color_dev on a device pointer with a row pitch -> host copy of the packed result"""
    from vision.devmat import DeviceMat
    scn, dcn = _channels(vp, name)
    ctx = vp.default_context()
    out = DeviceMat(ctx, (h, w) if dcn == 1 else (h, w, dcn))
    vp.check(vp.lib().vp_cvt_color_dev(ctx.handle, getattr(vp, name), ptr, stride, w, h, out.dev_ptr, None), ctx.handle)
    return out.host()


# ---- all 2^24 inputs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", THREE_CHANNEL_SOURCE)
def test_all_inputs_both_forms_interleaved_and_planes(vp, oracle, colours, name):
    exp = _expect(oracle, name, colours)
    dcn = _channels(vp, name)[1]
    ctx = vp.default_context()
    try:
        for form in (1, 0):
            ctx.set_option(vp.OPT_FLAT_OPS, form)
            got, _ = _cvt_u8(vp, name, colours)
            assert np.array_equal(got, exp), (name, form, "interleaved")
            if dcn != 3:
                continue
            _, planes = _cvt_u8(vp, name, colours, want_dst=False, planes_mask=7)
            for c in range(3):
                assert np.array_equal(planes[c], exp[:, :, c]), (name, form, "plane", c)
            if name == "RGB2LAB":                  # the Lab kernel has a form per wanted plane
                for c in range(3):
                    _, planes = _cvt_u8(vp, name, colours, want_dst=False, planes_mask=1 << c)
                    assert np.array_equal(planes[c], exp[:, :, c]), (name, form, "single plane", c)
    finally:
        ctx.set_option(vp.OPT_FLAT_OPS, 1)


# ---- tails, row pitch, alignment --------------------------------------------------------------------------------------------------------
def _random(rng, h, w, cn):
    return rng.integers(0, 256, (h, w) if cn == 1 else (h, w, cn), dtype=np.uint8)


@pytest.mark.parametrize("name", ALL_CODES)
def test_tails_pitch_and_alignment(vp, oracle, flat, name):
    """37 x 5 cut out of a 64-wide buffer one pixel in (row pitch, odd width, unaligned start) and 1 x 1: on the host path, and on the
    device path through the view's own device pointer; and the packed 37 x 5 image one pixel into a device buffer, where only the
    16-byte test keeps the 16-pixel form away."""
    from vision.devmat import DeviceMat
    scn, dcn = _channels(vp, name)
    ctx = vp.default_context()
    rng = np.random.default_rng(getattr(vp, name))
    big = _random(rng, 5, 64, scn)
    view = big[:, 1:38]
    one = _random(rng, 1, 1, scn)
    for img in (view, one, np.ascontiguousarray(view)):
        exp = _expect(oracle, name, img)
        got, planes = _cvt_u8(vp, name, img, planes_mask=7 if dcn == 3 else 0)
        assert got.shape == exp.shape and np.array_equal(got, exp), (name, img.shape)
        if dcn == 3:
            for c in range(3):
                assert np.array_equal(planes[c], exp[:, :, c]), (name, img.shape, c)
    dbig = DeviceMat.from_host(ctx, big)
    assert np.array_equal(_cvt_dev(vp, name, dbig.dev_ptr + scn, 64 * scn, 37, 5), _expect(oracle, name, view)), name
    done = DeviceMat.from_host(ctx, np.ascontiguousarray(np.broadcast_to(one, (1, 16) + one.shape[2:])))
    assert np.array_equal(_cvt_dev(vp, name, done.dev_ptr + scn, 16 * scn, 1, 1), _expect(oracle, name, one)), name
    packed = _random(rng, 1, 1 + 37 * 5, scn)                            # one pixel, then the 37 x 5 image with packed rows
    dpacked = DeviceMat.from_host(ctx, packed)
    img = packed[0, 1:].reshape((5, 37) if scn == 1 else (5, 37, scn))
    assert np.array_equal(_cvt_dev(vp, name, dpacked.dev_ptr + scn, 37 * scn, 37, 5), _expect(oracle, name, img)), name
    aligned = DeviceMat.from_host(ctx, np.ascontiguousarray(img))        # and aligned: the 16-pixel form with its tail of 185 % 16 pixels
    assert np.array_equal(_cvt_dev(vp, name, aligned.dev_ptr, 37 * scn, 37, 5), _expect(oracle, name, img)), name


@pytest.mark.parametrize("name", ALPHA)
def test_alpha_codes_on_a_wide_image(vp, oracle, flat, name):
    from vision.devmat import DeviceMat
    scn, dcn = _channels(vp, name)
    ctx = vp.default_context()
    img = _random(np.random.default_rng(100 + getattr(vp, name)), 8, 1920, scn)
    exp = _expect(oracle, name, img)
    assert np.array_equal(_cvt_u8(vp, name, img)[0], exp)
    if dcn == 3:                                   # the planes alone, no interleaved result
        _, planes = _cvt_u8(vp, name, img, want_dst=False, planes_mask=7)
        for c in range(3):
            assert np.array_equal(planes[c], exp[:, :, c]), (name, c)
    dm = DeviceMat.from_host(ctx, img)
    assert np.array_equal(_cvt_dev(vp, name, dm.dev_ptr, 1920 * scn, 1920, 8), exp)


# ---- the cv2 stand-in -------------------------------------------------------------------------------------------------------------------
FACADE = {"BGR2BGRA": "BGR2BGRA", "BGRA2BGR": "BGRA2BGR", "RGBA2RGB": "BGRA2BGR", "BGR2RGBA": "BGR2RGBA", "RGBA2BGR": "RGBA2BGR",
          "BGRA2RGB": "RGBA2BGR", "BGR2RGB": "BGR2RGB", "RGB2BGR": "BGR2RGB", "BGRA2RGBA": "BGRA2RGBA", "RGBA2BGRA": "BGRA2RGBA",
          "RGB2GRAY": "RGB2GRAY", "GRAY2BGRA": "GRAY2BGRA", "BGRA2GRAY": "BGRA2GRAY", "RGBA2GRAY": "RGBA2GRAY", "BGR2XYZ": "BGR2XYZ",
          "RGB2XYZ": "RGB2XYZ", "XYZ2BGR": "XYZ2BGR", "XYZ2RGB": "XYZ2RGB", "RGB2YCrCb": "RGB2YCRCB", "RGB2YCR_CB": "RGB2YCRCB",
          "YCrCb2BGR": "YCRCB2BGR", "YCR_CB2BGR": "YCRCB2BGR", "YCrCb2RGB": "YCRCB2RGB", "YCR_CB2RGB": "YCRCB2RGB", "RGB2HSV": "RGB2HSV",
          "RGB2Lab": "RGB2LAB", "RGB2LAB": "RGB2LAB", "RGB2HLS": "RGB2HLS", "HSV2RGB": "HSV2RGB", "Lab2RGB": "LAB2RGB", "LAB2RGB": "LAB2RGB",
          "HLS2BGR": "HLS2BGR", "HLS2RGB": "HLS2RGB", "BGR2YUV": "BGR2YUV", "RGB2YUV": "RGB2YUV", "YUV2BGR": "YUV2BGR", "YUV2RGB": "YUV2RGB"}


def test_bgr2yuv_through_the_facade_equals_the_restatement(vp):
    from vision import cv2_facade as cv2
    img = _random(np.random.default_rng(1), 45, 67, 3)
    from vision import devmat
    assert np.array_equal(np.asarray(cv2.cvtColor(img, cv2.COLOR_BGR2YUV)), R.bgr2yuv(img))
    lazy = devmat.lazy_enabled()
    devmat.set_lazy(False)                     # the mirror's host form: plain numpy in, plain numpy out
    try:
        got = cv2.cvtColor(img, cv2.COLOR_BGR2YUV)
        assert type(got) is np.ndarray and np.array_equal(got, R.bgr2yuv(img))
        bgra = cv2.cvtColor(img, cv2.COLOR_BGR2BGRA)
        assert type(bgra) is np.ndarray and np.array_equal(bgra, R.CODES["BGR2BGRA"](img))
        assert np.array_equal(cv2.cvtColor(bgra, cv2.COLOR_RGBA2RGB), img) and np.array_equal(cv2.cvtColor(bgra, cv2.COLOR_BGRA2GRAY), R.bgr2gray(img))
    finally:
        devmat.set_lazy(lazy)


def test_every_facade_value_reaches_its_code(vp, oracle):
    from vision import cv2_facade as cv2
    from vision.devmat import DeviceMat
    ctx = vp.default_context()
    rng = np.random.default_rng(2)
    assert set(FACADE.values()) == set(ALL_CODES)
    for cv_name, name in FACADE.items():
        scn, dcn = _channels(vp, name)
        img = _random(rng, 45, 67, scn)
        exp = _expect(oracle, name, img)
        got = cv2.cvtColor(img, getattr(cv2, "COLOR_" + cv_name))
        assert tuple(got.shape) == exp.shape and np.array_equal(np.asarray(got), exp), cv_name
        dm = DeviceMat.from_host(ctx, img)
        dgot = cv2.cvtColor(dm, getattr(cv2, "COLOR_" + cv_name))
        assert isinstance(dgot, DeviceMat), cv_name
        assert dm._host is None and dgot._host is None, f"{cv_name} made a host copy"
        assert np.array_equal(np.asarray(dgot), exp), cv_name


def test_mirror_wrappers_return_the_image_and_its_planes(vp):
    from vision.devmat import DeviceMat
    from vision.utils import color
    ctx = vp.default_context()
    img = _random(np.random.default_rng(3), 45, 67, 3)
    for fn, name in ((color.bgr_to_yuv, "BGR2YUV"), (color.yuv_to_bgr, "YUV2BGR"), (color.bgr_to_xyz, "BGR2XYZ"), (color.xyz_to_bgr, "XYZ2BGR"),
                     (color.ycrcb_to_bgr, "YCRCB2BGR"), (color.hls_to_bgr, "HLS2BGR")):
        exp = R.CODES[name](img)
        for src in (img, DeviceMat.from_host(ctx, img)):
            conv, planes = fn(src)
            assert np.array_equal(np.asarray(conv), exp) and len(planes) == 3, name
            for c in range(3):
                assert np.array_equal(np.asarray(planes[c]), exp[:, :, c]), (name, c)
            if isinstance(src, DeviceMat):
                assert isinstance(conv, DeviceMat) and all(isinstance(p, DeviceMat) for p in planes), name
    conv, planes = color._convert_colorspace(vp.BGR2BGRA)(img)
    assert tuple(conv.shape) == (45, 67, 4) and planes == ()


def test_hls_contrast_stretch_on_a_device_image(vp, oracle):
    """modules/color_balance.py:227-247: RGB2HLS, S and L clipped to their 0.2 / 99.8 percentiles and stretched to 0..255, HLS2RGB - the
    frame a DeviceMat, both conversions on the device."""
    from vision import cv2_facade as cv2
    from vision.devmat import DeviceMat
    import frames as F
    ctx = vp.default_context()
    rgb = np.ascontiguousarray(F.s1_buoy(2, 320, 180)[:, :, ::-1])

    def stretch(ch):
        ch = ch.astype(np.float64)
        lo, hi = np.percentile(ch, [0.2, 99.8])
        return ((np.clip(ch, lo, hi) - lo) * (255.0 / (hi - lo))).astype(np.uint8)

    frame = DeviceMat.from_host(ctx, rgb)
    hls = cv2.cvtColor(frame, cv2.COLOR_RGB2HLS)
    assert isinstance(hls, DeviceMat) and frame._host is None and hls._host is None
    h_ch, l_ch, s_ch = (np.asarray(p) for p in cv2.split(hls))
    edited = cv2.merge([h_ch, stretch(l_ch), stretch(s_ch)])
    out = cv2.cvtColor(DeviceMat.from_host(ctx, edited), cv2.COLOR_HLS2RGB)
    assert isinstance(out, DeviceMat)
    ohls = oracle.bgr2hls(R.swap_rb(rgb))
    exp = R.swap_rb(R.hls2bgr(np.dstack([ohls[..., 0], stretch(ohls[..., 1]), stretch(ohls[..., 2])])))
    assert np.array_equal(np.asarray(hls), ohls)
    assert np.array_equal(np.asarray(out), exp)


# ---- what still raises ------------------------------------------------------------------------------------------------------------------
def test_unchanged_refusals(vp):
    from vision import cv2_facade as cv2
    bgr = np.zeros((4, 4, 3), np.uint8)
    bgra = np.zeros((4, 4, 4), np.uint8)
    with pytest.raises(cv2.error):
        cv2.cvtColor(bgr, cv2.COLOR_BGR2LUV)
    for unknown in (51, 86, 127, 1000, -1):
        with pytest.raises(cv2.error):
            cv2.cvtColor(bgr, unknown)
    with pytest.raises(ValueError):
        cv2.cvtColor(bgr, cv2.COLOR_BGRA2BGR)          # three channels where four are needed
    with pytest.raises(ValueError):
        cv2.cvtColor(bgra, cv2.COLOR_BGR2YUV)
    with pytest.raises(ValueError):
        cv2.cvtColor(bgr[:, :, 0], cv2.COLOR_RGB2GRAY)
    ctx = vp.default_context()
    L = vp.lib()
    three = (vp.C.c_void_p * 3)(vp.ptr(bgr), None, None)
    out = np.zeros((4, 4, 4), np.uint8)
    for name in ("BGR2BGRA", "BGR2RGBA", "BGRA2RGBA", "GRAY2BGRA", "BGRA2GRAY", "RGBA2GRAY", "RGB2GRAY"):      # planes with a 1- or 4-channel result
        assert L.vp_cvt_color_u8(ctx.handle, getattr(vp, name), vp.ptr(bgra), 16, 4, 4, vp.ptr(out), three) == -1, name
        assert L.vp_cvt_color_dev(ctx.handle, getattr(vp, name), vp.ptr(bgra), 16, 4, 4, vp.ptr(out), three) == -1, name
    assert L.vp_cvt_color_u8(ctx.handle, vp.CVT_CODES, vp.ptr(bgra), 16, 4, 4, vp.ptr(out), None) == -1
    assert L.vp_cvt_color_u8(ctx.handle, -1, vp.ptr(bgra), 16, 4, 4, vp.ptr(out), None) == -1
    assert L.vp_cvt_color_u8(ctx.handle, vp.BGRA2BGR, vp.ptr(bgra), 15, 4, 4, vp.ptr(out), None) == -1      # stride below four bytes per pixel
    assert L.vp_cvt_color_u8(ctx.handle, vp.BGRA2BGR, vp.ptr(bgra), 16, 4, 4, None, None) == -1             # nowhere to put the result
    assert not out.any()
