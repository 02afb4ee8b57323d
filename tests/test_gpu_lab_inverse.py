"""GPU: Lab -> BGR (VP_LAB2BGR) and the two white balances, bit-equal to the restatement (tests/lab_inverse_restate.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frames as F  # noqa: E402
import lab_inverse_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _all_lab():
    """(4096, 4096, 3): every 8-bit (L, a, b) once."""
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


@pytest.fixture(scope="module")
def all_lab():
    lab = _all_lab()
    return lab, R.lab2bgr(lab)


@pytest.fixture(params=[1, 0], ids=["flat", "generic"])
def flat(request, vp):
    ctx = vp.default_context()
    ctx.set_option(vp.OPT_FLAT_OPS, request.param)
    yield request.param
    ctx.set_option(vp.OPT_FLAT_OPS, 1)


def _cvt_u8(vp, src, planes_mask, want_dst=True):
    h, w = src.shape[:2]
    dst = np.zeros((h, w, 3), np.uint8) if want_dst else None
    planes = [np.zeros((h, w), np.uint8) if planes_mask & (1 << c) else None for c in range(3)]
    arr = (vp.C.c_void_p * 3)(*[vp.ptr(p) for p in planes])
    ctx = vp.default_context()
    vp.check(vp.lib().vp_cvt_color_u8(ctx.handle, vp.LAB2BGR, vp.ptr(src), src.strides[0], w, h, vp.ptr(dst), arr if planes_mask else None),
             ctx.handle)
    return dst, planes


def test_all_inputs_host_device_facade(vp, flat, all_lab):
    from vision import cv2_facade as cv2
    from vision.devmat import DeviceMat
    from vision.utils import color
    lab, exp = all_lab
    got, planes = color.lab_to_bgr(lab)
    assert np.array_equal(got, exp)
    for c in range(3):
        assert np.array_equal(planes[c], exp[:, :, c])
    assert np.array_equal(cv2.cvtColor(lab, cv2.COLOR_LAB2BGR), exp) and cv2.COLOR_Lab2BGR == 56
    ctx = vp.default_context()
    dm = DeviceMat.from_host(ctx, lab)
    dgot, dplanes = color.lab_to_bgr(dm)
    assert isinstance(dgot, DeviceMat)
    assert np.array_equal(dgot.host(), exp)
    for c in range(3):
        assert np.array_equal(dplanes[c].host(), exp[:, :, c])


@pytest.mark.parametrize("mask", [1, 2, 4, 3, 5, 6, 7])
def test_plane_subsets(vp, flat, all_lab, mask):
    lab, exp = all_lab                            # every subset of planes on all 2^24 inputs
    dst, planes = _cvt_u8(vp, lab, mask, want_dst=False)
    for c in range(3):
        if mask & (1 << c):
            assert np.array_equal(planes[c], exp[:, :, c]), c


@pytest.mark.parametrize("hw", [(1, 1), (1, 17), (3, 5), (17, 33), (31, 61), (241, 319), (1080, 1920)])
def test_ragged_and_strided(vp, flat, hw):
    rng = np.random.default_rng(hw[0] * 7 + hw[1])
    h, w = hw
    big = rng.integers(0, 256, (h, w + 5, 3), dtype=np.uint8)
    view = big[:, 2:2 + w]                       # a row pitch wider than the row, unaligned start
    got, _ = _cvt_u8(vp, view, 7)
    assert np.array_equal(got, R.lab2bgr(view))
    from vision.utils import color
    assert np.array_equal(color.lab_to_bgr(view)[0], R.lab2bgr(view))


def _frame(h, w, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[..., 0] = (img[..., 0] // 3).astype(np.uint8)      # a colour cast
    img[..., 2] = np.minimum(255, img[..., 2].astype(np.int32) + 60).astype(np.uint8)
    return img


def _check_global(vp, oracle, bgr):
    from vision.utils import color
    lab = oracle.bgr2lab(np.ascontiguousarray(bgr))
    exp, (ea, eb) = R.white_balance_bgr(lab)
    means = np.zeros(2, np.float32)
    got = color.white_balance_bgr(bgr, ab_mean_out=means)
    assert means[0] == np.mean(lab[..., 1].astype(np.float32)) and means[1] == np.mean(lab[..., 2].astype(np.float32))
    assert means[0] == ea and means[1] == eb
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (97, 211), (1081, 1917), (1080, 1920), (2160, 3840)])
def test_white_balance_global(vp, oracle, hw):
    _check_global(vp, oracle, _frame(*hw, seed=hw[0]))


def test_white_balance_global_near_integer_means(vp, oracle):
    """Planes whose mean sits on or next to an integer: the shift (mean - 128) decides the truncation of every pixel."""
    base = np.full((1080, 1920, 3), (90, 120, 150), np.uint8)
    _check_global(vp, oracle, base)
    for k in (1, 2, 3, 8191, 8192, 8193):
        img = base.copy()
        img.reshape(-1, 3)[:k] = (200, 60, 40)
        _check_global(vp, oracle, img)
    _check_global(vp, oracle, F.s1_buoy(0, 1920, 1080))
    _check_global(vp, oracle, _frame(300, 410, 5)[::2, 3:400])   # a view with a row pitch wider than its rows (host path stride)


def _wrap_counts(v):
    return int((v >= 256).sum()), int((v < 0).sum()), int(((v < 0) & (v > -1)).sum())


def _wrap_frame_global():
    """A green frame with a small magenta patch: a' reaches 296.3 and b' falls to -0.73 - the astype(np.uint8) wrap on both sides,
    and truncation toward zero (not floor) for values in (-1, 0)."""
    img = np.zeros((64, 96, 3), np.uint8)
    img[:] = (0, 200, 0)
    img[20:26, 40:50] = (255, 0, 255)
    return img


def _wrap_frame_blur(h=120, w=160):
    """Green with isolated magenta pixels, a magenta block and isolated green pixels inside it: pixels far from their box mean."""
    img = np.zeros((h, w, 3), np.uint8)
    img[:] = (0, 200, 0)
    img[::9, ::11] = (255, 0, 255)
    img[h // 2:, :w // 3] = (255, 0, 255)
    img[h // 2 + 3::7, 2:w // 3:7] = (0, 200, 0)
    return img


def test_white_balance_global_wraps(vp, oracle):
    bgr = _wrap_frame_global()
    a, b = R.white_balance_ab(oracle.bgr2lab(bgr))
    assert _wrap_counts(a)[0] == 60 and _wrap_counts(b)[1:] == (60, 60)      # the restatement really wraps here
    _check_global(vp, oracle, bgr)


@pytest.mark.parametrize("k", [3, 5, 31, 255])
def test_white_balance_blur_wraps(vp, oracle, k):
    from vision.utils import color
    bgr = _wrap_frame_blur()
    lab = oracle.bgr2lab(bgr)
    a, b = R.white_balance_ab(lab, k)
    ca, cb = _wrap_counts(a), _wrap_counts(b)
    assert ca[0] > 0 and (ca[1] > 0 or k == 255)                             # above 255 and below 0
    if k == 31:
        assert ca[2] + cb[2] > 0                                             # values in (-1, 0): truncation, not floor
    assert np.array_equal(color.white_balance_bgr_blur(bgr, k), R.white_balance_bgr_blur(lab, k))


def test_white_balance_dev_row_pitch(vp, oracle):
    """vp_white_balance_dev with src_stride > 3 w (the Python entry points pass packed device images): both forms."""
    from vision.devmat import DeviceMat
    ctx = vp.default_context()
    h, w, pad = 97, 211, 7
    big = _wrap_frame_blur(h, w + pad)
    view = big[:, 3:3 + w]
    lab = oracle.bgr2lab(np.ascontiguousarray(view))
    src = DeviceMat.from_host(ctx, big)
    base = src.dev_ptr + 3 * 3                    # column 3 of the wide rows
    for k, exp in ((vp.WB_GLOBAL_MEAN, R.white_balance_bgr(lab)[0]), (31, R.white_balance_bgr_blur(lab, 31))):
        dst = DeviceMat(ctx, (h, w, 3))
        vp.check(vp.lib().vp_white_balance_dev(ctx.handle, base, (w + pad) * 3, w, h, k, dst.dev_ptr, None), ctx.handle)
        assert np.array_equal(dst.host(), exp), k


@pytest.mark.parametrize("k", [1, 3, 5, 31, 255])
def test_white_balance_blur(vp, oracle, k):
    from vision.utils import color
    for h, w in [(1, 1), (7, 5), (97, 211), (1080, 1920)]:
        bgr = _frame(h, w, seed=k + h)
        lab = oracle.bgr2lab(bgr)
        assert np.array_equal(color.white_balance_bgr_blur(bgr, k), R.white_balance_bgr_blur(lab, k)), (h, w)
    if k > 1:      # an even size rounds up, as in the reference
        assert np.array_equal(color.white_balance_bgr_blur(bgr, k - 1), R.white_balance_bgr_blur(lab, k))


def test_white_balance_blur_kernel_larger_than_image(vp, oracle):
    from vision.utils import color
    for (h, w), k in [((3, 4), 9), ((20, 13), 101), ((64, 300), 255), ((1, 1), 4095)]:
        bgr = _frame(h, w, seed=h)
        lab = oracle.bgr2lab(bgr)
        assert np.array_equal(color.white_balance_bgr_blur(bgr, k), R.white_balance_bgr_blur(lab, k)), (h, w, k)
    view = _frame(200, 260, 9)[5:150, 7:250]       # a row pitch wider than the rows: the host path passes it as src_stride
    assert np.array_equal(color.white_balance_bgr_blur(view, 31), R.white_balance_bgr_blur(oracle.bgr2lab(np.ascontiguousarray(view)), 31))
    with pytest.raises(vp.VpError):
        color.white_balance_bgr_blur(bgr, 4097)


def test_white_balance_device_resident(vp, oracle):
    from vision.devmat import DeviceMat
    from vision.utils import color
    ctx = vp.default_context()
    bgr = _frame(720, 1280, 3)
    lab = oracle.bgr2lab(bgr)
    dm = DeviceMat.from_host(ctx, bgr)
    g = color.white_balance_bgr(dm)
    b = color.white_balance_bgr_blur(dm, 5)
    assert isinstance(g, DeviceMat) and isinstance(b, DeviceMat)
    assert np.array_equal(g.host(), R.white_balance_bgr(lab)[0])
    assert np.array_equal(b.host(), R.white_balance_bgr_blur(lab, 5))


def test_auto_calibrate_lab_to_bgr_calls(vp, oracle):
    """modules/auto_calibrate.py process(): bgr_to_lab, then lab_to_bgr of (L, 128, 128) and of (128, a, b), with numpy frames and
    with DeviceMat frames."""
    from vision import cv2_facade as cv2
    from vision.devmat import DeviceMat
    from vision.utils.color import bgr_to_lab, lab_to_bgr
    img = F.s1_buoy(3, 1280, 720)
    ctx = vp.default_context()
    for frame in (img, DeviceMat.from_host(ctx, img)):
        _, lab_img = bgr_to_lab(frame)
        lab_l, lab_a, lab_b = (np.asarray(p) for p in lab_img)
        bgr_lab_l, (_, _, _) = lab_to_bgr(cv2.merge([lab_l, np.zeros_like(lab_l) + 128, np.zeros_like(lab_l) + 128]))
        bgr_lab_ab, (_, _, _) = lab_to_bgr(cv2.merge([np.zeros_like(lab_a) + 128, lab_a, lab_b]))
        lab = oracle.bgr2lab(img)
        exp_l = R.lab2bgr(np.dstack([lab[..., 0], np.full_like(lab[..., 0], 128), np.full_like(lab[..., 0], 128)]))
        exp_ab = R.lab2bgr(np.dstack([np.full_like(lab[..., 0], 128), lab[..., 1], lab[..., 2]]))
        assert np.array_equal(np.asarray(bgr_lab_l), exp_l)
        assert np.array_equal(np.asarray(bgr_lab_ab), exp_ab)
