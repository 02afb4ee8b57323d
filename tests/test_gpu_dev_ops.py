"""GPU suite for the operators that now keep a device image on the device: Gaussian blur (both kernels), resize, warpAffine / rotate /
translate, cv2.threshold and its mirror wrappers, Otsu, the mean adaptive threshold, simple_canny's statistic and the labelling.

Every comparison is bit-exact.  Expectations come from the CPU oracle and from the restatements the host forms are pinned to
(tests/resize_restate.py, the numpy statement of cv2.threshold, the float64 Otsu scan), never from the library under test."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import frames as F
import resize_restate as RR

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 7), (7, 1), (67, 45), (640, 360), (1920, 1080)]     # (w, h)
SMALL = SHAPES[:4]
HERE = os.path.dirname(os.path.abspath(__file__))


def _img(rng, w, h, cn):
    """A smooth scene plus noise (so that blurs, warps and thresholds all have structure to act on)."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = (96 + 80 * np.sin(xx / 37.0 + cn) * np.cos(yy / 23.0))[..., None] + np.arange(cn) * 17
    img = np.clip(base + rng.normal(0, 25, (h, w, cn)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(img[:, :, 0]) if cn == 1 else img


def _dev(ctx, arr):
    from vision.devmat import DeviceMat
    return DeviceMat.from_host(ctx, arr)


def _same(a, b):
    """array_equal for centroid tables: the background row of a mask without background pixels is (nan, nan) on both sides"""
    return np.array_equal(a, b, equal_nan=True)


def _resident(*mats):
    from vision.devmat import DeviceMat
    for m in mats:
        assert isinstance(m, DeviceMat), type(m)
        assert m._host is None, "an image was downloaded although nothing read it"


def _device_gray(ctx, w, h, seed=3):
    """A single-channel image that a device operator produced, and its host expectation."""
    from vision.utils.color import bgr_to_gray
    bgr = F.s1_buoy(seed, w, h)
    gray = bgr_to_gray(_dev(ctx, bgr))[0]
    _resident(gray)
    return gray, bgr


# ---- Gaussian blur -------------------------------------------------------------------------------------------------------------------
KERNELS = [(1, 1), (3, 3), (5, 5), (7, 7), (11, 11), (31, 31), (33, 33), (51, 51), (5, 1), (1, 9), (3, 15)]


def _blur_cases():
    cases = []
    for (w, h) in SMALL:                                   # images narrower and shorter than the kernel radius among them
        for cn in (1, 3, 4):
            for k in KERNELS:
                for sigma in (0.0, 1.7):
                    cases.append((w, h, cn, k, sigma))
    for i, k in enumerate(KERNELS):
        cases.append((640, 360, 3, k, (0.0, 1.7)[i & 1]))
        cases.append((640, 360, 1, k, (1.7, 0.0)[i & 1]))
        cases.append((640, 360, 4, k, 0.0))
        cases.append((1920, 1080, 3, k, 0.0))
        cases.append((1920, 1080, 1, k, 1.7))
    return cases


def test_gaussian_blur_dev_both_kernels_equal_the_oracle(vp, oracle):
    """Every case under VP_OPT_BLUR_ONEPASS 1 (the one-pass kernel wherever its tile fits: kernels up to 31), 0 (always two passes) and
    the default: all three equal the oracle, whatever the dispatch chooses."""
    from vision import cv2_facade
    ctx = vp.default_context()
    rng = np.random.default_rng(11)
    try:
        for (w, h, cn, k, sigma) in _blur_cases():
            img = _img(rng, w, h, cn)
            exp = oracle.gaussian_blur(img, k, sigma, 0.0)
            src = _dev(ctx, img)
            for opt in (1, 0, -1):
                ctx.set_option(vp.OPT_BLUR_ONEPASS, opt)
                out = cv2_facade.GaussianBlur(src, k, sigma)
                _resident(src, out)
                assert out.shape == img.shape
                assert np.array_equal(np.asarray(out), exp), (w, h, cn, k, sigma, opt)
    finally:
        ctx.set_option(vp.OPT_BLUR_ONEPASS, -1)


def test_gaussian_blur_mirror_and_numpy_callers(vp, oracle):
    from vision import cv2_facade
    from vision.utils.transform import simple_gaussian_blur
    ctx = vp.default_context()
    rng = np.random.default_rng(12)
    img = _img(rng, 640, 360, 3)
    exp = oracle.gaussian_blur(img, (5, 5), 0.0, 0.0)
    src = _dev(ctx, img)
    out = simple_gaussian_blur(src, 5, 0)
    _resident(src, out)
    assert np.array_equal(np.asarray(out), exp)
    host = simple_gaussian_blur(img, 5, 0)                # nothing changed for host callers
    assert type(host) is np.ndarray and np.array_equal(host, exp)
    host = cv2_facade.GaussianBlur(img, (9, 3), 2.0, None, 0.5)
    assert type(host) is np.ndarray and np.array_equal(host, oracle.gaussian_blur(img, (9, 3), 2.0, 0.5))
    out = cv2_facade.GaussianBlur(src, (9, 3), 2.0, None, 0.5)
    _resident(out)
    assert np.array_equal(np.asarray(out), host)
    # _into keeps working: the result lands in dst
    dst = np.zeros_like(img)
    r = cv2_facade.GaussianBlur(src, (5, 5), 0, dst)
    assert r is dst and np.array_equal(dst, exp)
    # the exceptions of the host branch, word for word
    for bad, kwargs in (((4, 4), {}), ((5, 5), {"borderType": 1})):
        msgs = []
        for s in (img, src):
            with pytest.raises(cv2_facade.error) as e:
                cv2_facade.GaussianBlur(s, bad, 0, **kwargs)
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1]
    with pytest.raises(ValueError):
        simple_gaussian_blur(src, 4, 0)


def test_strided_sources_through_the_c_abi(vp, oracle):
    """A column window of a wider device buffer: src_stride is honoured by every entry that takes one."""
    ctx = vp.default_context()
    L = vp.lib()
    rng = np.random.default_rng(13)
    from vision.devmat import DeviceMat
    for cn in (1, 3, 4):
        W, h, x0, w = 200, 45, 31, 67
        wide = _img(rng, W, h, cn)
        win = np.ascontiguousarray(wide[:, x0:x0 + w])
        dwide = _dev(ctx, wide)
        sp = dwide.dev_ptr + x0 * cn
        try:
            for opt in (1, 0):
                ctx.set_option(vp.OPT_BLUR_ONEPASS, opt)
                for k in ((5, 5), (31, 31), (33, 33), (3, 15)):
                    out = DeviceMat(ctx, win.shape)
                    vp.check(L.vp_gaussian_blur_dev(ctx.handle, sp, W * cn, w, h, cn, k[0], k[1], 0.0, 0.0, out.dev_ptr), ctx.handle)
                    assert np.array_equal(np.asarray(out), oracle.gaussian_blur(win, k, 0.0, 0.0)), (cn, k, opt)
        finally:
            ctx.set_option(vp.OPT_BLUR_ONEPASS, -1)
        for (dw, dh) in ((40, 30), (67, 45), (131, 77)):
            out = DeviceMat(ctx, (dh, dw) if cn == 1 else (dh, dw, cn))
            vp.check(L.vp_resize_dev(ctx.handle, sp, W * cn, w, h, cn, dw, dh, 0.0, 0.0, out.dev_ptr), ctx.handle)
            assert np.array_equal(np.asarray(out), RR.resize(win, dsize=(dw, dh))), (cn, dw, dh)
        M = oracle.rotation_matrix_2d((w / 2, h / 2), 17.0, 0.9)
        m = np.ascontiguousarray(M, np.float64)
        bv = np.array([9, 8, 7, 6], np.uint8)
        for border, name in ((0, "constant"), (1, "replicate")):
            out = DeviceMat(ctx, (50, 70) if cn == 1 else (50, 70, cn))
            vp.check(L.vp_warp_affine_dev(ctx.handle, sp, W * cn, w, h, cn, m.ctypes.data, 0, border, bv.ctypes.data, out.dev_ptr, 70, 50), ctx.handle)
            assert np.array_equal(np.asarray(out), oracle.warp_affine(win, M, (70, 50), border=name, value=bv[:cn] if cn > 1 else 9)), (cn, name)
        if cn == 1:
            out = DeviceMat(ctx, win.shape)
            vp.check(L.vp_adaptive_threshold_mean_dev(ctx.handle, sp, W, w, h, 255.0, 0, 11, 3.0, out.dev_ptr), ctx.handle)
            assert np.array_equal(np.asarray(out), oracle.adaptive_threshold_mean(win, 255, False, 11, 3.0))
            mask = np.where(win > 120, 255, 0).astype(np.uint8)
            wide_mask = np.where(wide > 120, 255, 0).astype(np.uint8)
            dm = _dev(ctx, wide_mask)
            labels = DeviceMat(ctx, (h, w), np.int32)
            stats = np.empty((4096, 5), np.int32)
            cent = np.empty((4096, 2), np.float64)
            n = C.c_int32(0)
            vp.check(L.vp_ccl_dev(ctx.handle, dm.dev_ptr + x0, W, w, h, 2, labels.dev_ptr, stats.ctypes.data, cent.ctypes.data, 4096, C.byref(n)),
                     ctx.handle)
            rn, rl, rs, rc = oracle.ccl(mask, 2)
            assert n.value == rn and np.array_equal(np.asarray(labels), rl) and np.array_equal(stats[:rn], rs) and _same(cent[:rn], rc)
    # argument checks of the host forms, and the overlap rule
    img = _dev(ctx, _img(rng, 16, 16, 1))
    out = DeviceMat(ctx, (16, 16))
    assert L.vp_gaussian_blur_dev(ctx.handle, img.dev_ptr, 16, 16, 16, 1, 4, 5, 0.0, 0.0, out.dev_ptr) == -1
    assert L.vp_gaussian_blur_dev(ctx.handle, img.dev_ptr, 16, 16, 16, 1, 513, 5, 0.0, 0.0, out.dev_ptr) == -1
    assert L.vp_gaussian_blur_dev(ctx.handle, img.dev_ptr, 15, 16, 16, 1, 5, 5, 0.0, 0.0, out.dev_ptr) == -1
    assert L.vp_gaussian_blur_dev(ctx.handle, img.dev_ptr, 16, 16, 16, 1, 5, 5, 0.0, 0.0, img.dev_ptr) == -1
    assert L.vp_gaussian_blur_dev(ctx.handle, img.dev_ptr, 16, 16, 65536, 1, 5, 5, 0.0, 0.0, out.dev_ptr) == -1
    assert L.vp_threshold_u8_dev(ctx.handle, img.dev_ptr, 256, 10.0, 255.0, 5, out.dev_ptr) == -1
    assert L.vp_threshold_u8_dev(ctx.handle, img.dev_ptr, 256, 10.0, 255.0, 0, img.dev_ptr + 8) == -1
    assert L.vp_adaptive_threshold_mean_dev(ctx.handle, img.dev_ptr, 16, 16, 16, 255.0, 0, 4, 0.0, out.dev_ptr) == -1
    assert L.vp_adaptive_threshold_mean_dev(ctx.handle, img.dev_ptr, 16, 16, 16, 255.0, 0, 153, 0.0, out.dev_ptr) == -4
    assert L.vp_resize_dev(ctx.handle, img.dev_ptr, 16, 16, 16, 1, 0, 8, 0.0, 0.0, out.dev_ptr) == -1
    assert L.vp_hist_u8_dev(ctx.handle, img.dev_ptr, 0, stats.ctypes.data) == -1
    assert L.vp_ccl_dev(ctx.handle, img.dev_ptr, 16, 16, 16, 7, None, None, None, 16, C.byref(n)) == -1


# ---- resize, warp -----------------------------------------------------------------------------------------------------------------------
def test_resize_dev_equals_the_restatement(vp):
    from vision import cv2_facade
    from vision.utils import transform
    ctx = vp.default_context()
    rng = np.random.default_rng(14)
    for (w, h) in SHAPES:
        for cn in (1, 3, 4):
            if (w, h) == (1920, 1080) and cn == 4:
                continue
            img = _img(rng, w, h, cn)
            src = _dev(ctx, img)
            sizes = [(max(1, w // 2 + 1), max(1, h // 3 + 1)), (w + 5, h + 3), (w, h)]
            if w % 2 == 0 and h % 2 == 0:
                sizes.append((w // 2, h // 2))            # the exact halving (OpenCV's 2x2 box average)
            for dsize in sizes:
                exp = RR.resize(img, dsize=dsize)
                out = cv2_facade.resize(src, dsize)
                _resident(src, out)
                assert np.array_equal(np.asarray(out), exp), (w, h, cn, dsize)
                if (w, h) in SMALL:
                    host = cv2_facade.resize(img, dsize)
                    assert type(host) is np.ndarray and np.array_equal(host, exp)
            if w >= 7 and h >= 7:
                exp = RR.resize(img, fx=0.37, fy=1.6)
                out = cv2_facade.resize(src, None, fx=0.37, fy=1.6)
                _resident(src, out)
                assert np.array_equal(np.asarray(out), exp), (w, h, cn)
    img = _img(rng, 67, 45, 3)
    src = _dev(ctx, img)
    out = transform.resize(src, 40, 30)
    _resident(src, out)
    assert np.array_equal(np.asarray(out), RR.resize(img, dsize=(40, 30)))
    assert type(transform.resize(img, 40, 30)) is np.ndarray
    msgs = []
    for s in (img, src):
        with pytest.raises(cv2_facade.error) as e:
            cv2_facade.resize(s, (0, 5))
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1]
    odd = _dev(ctx, _img(rng, 67, 45, 1))
    with pytest.raises(cv2_facade.error):                  # scale 2 with a partial edge cell: not reproduced, as in the host form
        cv2_facade.resize(odd, None, fx=0.5, fy=0.5)


def test_warp_affine_rotate_translate_dev_equal_the_oracle(vp, oracle):
    from vision import cv2_facade
    from vision.utils import transform
    ctx = vp.default_context()
    rng = np.random.default_rng(15)
    for (w, h) in SHAPES:
        for cn in (1, 3, 4):
            if (w, h) == (1920, 1080) and cn == 4:
                continue
            img = _img(rng, w, h, cn)
            src = _dev(ctx, img)
            M = oracle.rotation_matrix_2d((w / 2, h / 2), 23.5, 1.1)
            out = cv2_facade.warpAffine(src, M, (w + 3, h + 2), None, cv2_facade.INTER_LINEAR, cv2_facade.BORDER_CONSTANT, (5, 6, 7, 8))
            _resident(src, out)
            exp = oracle.warp_affine(img, M, (w + 3, h + 2), border="constant", value=(5, 6, 7, 8)[:cn] if cn > 1 else 5)
            assert np.array_equal(np.asarray(out), exp), (w, h, cn)
            out = cv2_facade.warpAffine(src, M, (w, h), flags=cv2_facade.INTER_LINEAR | cv2_facade.WARP_INVERSE_MAP, borderMode=cv2_facade.BORDER_REPLICATE)
            _resident(src, out)
            assert np.array_equal(np.asarray(out), oracle.warp_affine(img, M, (w, h), inverse_map=True, border="replicate")), (w, h, cn)
            rot = transform.rotate(src, 30.0)
            _resident(src, rot)
            Mr = oracle.rotation_matrix_2d((w / 2, h / 2), 30.0, 1.0)
            exp = oracle.warp_affine(img, Mr, (w, h), border="replicate")
            assert np.array_equal(np.asarray(rot), exp), (w, h, cn)
            tr = transform.translate(src, 3, -2)
            _resident(src, tr)
            exp_t = oracle.warp_affine(img, np.float32([[1, 0, 3], [0, 1, -2]]), (w, h))
            assert np.array_equal(np.asarray(tr), exp_t), (w, h, cn)
            if (w, h) in SMALL:
                host = transform.rotate(img, 30.0)
                assert type(host) is np.ndarray and np.array_equal(host, exp)
                host = transform.translate(img, 3, -2)
                assert type(host) is np.ndarray and np.array_equal(host, exp_t)
    msgs = []
    img = _img(rng, 20, 10, 3)
    for s in (img, _dev(ctx, img)):
        with pytest.raises(cv2_facade.error) as e:
            cv2_facade.warpAffine(s, np.eye(3), (20, 10))
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1]


# ---- thresholds -----------------------------------------------------------------------------------------------------------------------
def _np_threshold(img, thresh, maxval, kind):
    """The numpy statement of cv2.threshold on 8-bit data: compare with floor(thresh); maxval rounded half to even and saturated."""
    t = math.floor(thresh)
    m = int(min(255, max(0, np.rint(maxval))))
    v = img.astype(np.int64)
    above = v > t
    if kind == 0:
        out = np.where(above, m, 0)
    elif kind == 1:
        out = np.where(above, 0, m)
    elif kind == 2:
        out = np.where(above, min(255, max(0, t)), v)
    elif kind == 3:
        out = np.where(above, v, 0)
    else:
        out = np.where(above, 0, v)
    return out.astype(np.uint8)


def test_threshold_dev_equals_the_numpy_statement(vp):
    from vision import cv2_facade
    from vision.utils import color
    ctx = vp.default_context()
    rng = np.random.default_rng(16)
    for (w, h) in SHAPES:
        for cn in (1, 3, 4):
            if (w, h) == (1920, 1080) and cn == 4:
                continue
            img = _img(rng, w, h, cn)
            src = _dev(ctx, img)
            for kind in range(5):
                for thresh, maxval in ((100, 255), (127.9, 200.5), (-3, 255), (300, 255), (0, 254.5)):
                    if (w, h) not in SMALL and (thresh, maxval) not in ((100, 255), (127.9, 200.5)):
                        continue
                    exp = _np_threshold(img, thresh, maxval, kind)
                    rv, out = cv2_facade.threshold(src, thresh, maxval, kind)
                    _resident(src, out)
                    assert rv == float(thresh) and out.shape == img.shape
                    assert out.binary == (kind in (0, 1) and cn == 1 and maxval == 255), "0 / 255 masks take the bit paths downstream"
                    assert np.array_equal(np.asarray(out), exp), (w, h, cn, kind, thresh, maxval)
                    if (w, h) in SMALL:
                        rv, host = cv2_facade.threshold(img, thresh, maxval, kind)
                        assert rv == float(thresh) and type(host) is np.ndarray and np.array_equal(host, exp)
            for fn, kind in ((color.max_threshold, 2), (color.above_threshold, 3), (color.below_threshold, 4)):
                out = fn(src, 117.5)
                _resident(src, out)
                exp = _np_threshold(img, 117.5, 0, kind)
                assert np.array_equal(np.asarray(out), exp), (w, h, cn, kind)
                if (w, h) in SMALL:
                    host = fn(img, 117.5)
                    assert type(host) is np.ndarray and np.array_equal(host, exp)
    with pytest.raises(TypeError) as e1:
        color.max_threshold(np.zeros((4, 4), np.float32), 3)
    from vision.devmat import DeviceMat
    with pytest.raises(TypeError) as e2:
        color.max_threshold(DeviceMat.from_host(ctx, np.zeros((4, 4), np.float32)), 3)
    assert str(e1.value) == str(e2.value)


def _otsu_expectation(img):
    """getThreshVal_Otsu_8u restated in float64 (the scan tests/test_gpu_parity.py::test_otsu_threshold pins the host form to)."""
    h = np.bincount(img.ravel(), minlength=256).astype(np.float64)
    scale = 1.0 / img.size
    mu = float((np.arange(256) * h).sum()) * scale
    mu1 = q1 = 0.0
    best, arg = 0.0, 0.0
    for i in range(256):
        p = h[i] * scale
        mu1 *= q1
        q1 += p
        q2 = 1.0 - q1
        if min(q1, q2) < 1.1920929e-07 or max(q1, q2) > 1.0 - 1.1920929e-07:
            continue
        mu1 = (mu1 + i * p) / q1
        mu2 = (mu - q1 * mu1) / q2
        s = q1 * q2 * (mu1 - mu2) ** 2
        if s > best:
            best, arg = s, float(i)
    return arg


def test_otsu_dev_threshold_and_image(vp):
    from vision import cv2_facade
    from vision.utils import color
    ctx = vp.default_context()
    rng = np.random.default_rng(5)
    known = json.load(open(os.path.join(HERE, "golden", "known_answers.json")))["otsu_two_values"]
    two = np.repeat(np.array([known["values"]], np.uint8), 6, 0)
    yy, xx = np.mgrid[0:2160, 0:3840]
    big = np.clip(np.where((xx // 480 + yy // 270) % 2 == 0, 70, 170) + rng.normal(0, 18, (2160, 3840)), 0, 255).astype(np.uint8)
    cases = [rng.integers(0, 256, (77, 91), dtype=np.uint8),
             np.clip(np.concatenate([rng.normal(60, 12, 4000), rng.normal(180, 20, 6000)]), 0, 255).astype(np.uint8).reshape(100, 100),
             np.full((8, 8), 7, np.uint8), two, np.array([[133]], np.uint8), big,
             _img(rng, 67, 45, 1), _img(rng, 640, 360, 1), _img(rng, 1920, 1080, 1), _img(rng, 1, 7, 1), _img(rng, 7, 1, 1)]
    for img in cases:
        arg = _otsu_expectation(img)
        if img is two:
            assert arg == known["threshold"]
        src = _dev(ctx, img)
        t, out = color.otsu_threshold(src)
        _resident(src, out)
        assert isinstance(t, float) and t == arg, (img.shape, t, arg)
        assert out.binary
        assert np.array_equal(np.asarray(out), np.where(img > arg, 255, 0).astype(np.uint8)), img.shape
        th, host = color.otsu_threshold(img)
        assert th == arg and type(host) is np.ndarray and np.array_equal(host, np.asarray(out))
        for kind in (1, 2, 3, 4):
            rv, o2 = cv2_facade.threshold(src, 0, 200, kind | cv2_facade.THRESH_OTSU)
            _resident(src, o2)
            assert rv == arg and np.array_equal(np.asarray(o2), _np_threshold(img, arg, 200, kind)), (img.shape, kind)
        rv, h2 = cv2_facade.threshold(img, 0, 255, cv2_facade.THRESH_OTSU)
        assert rv == arg and type(h2) is np.ndarray and np.array_equal(h2, host)


def test_adaptive_mean_dev_equals_the_oracle(vp, oracle):
    from vision import cv2_facade
    from vision.utils import color
    ctx = vp.default_context()
    rng = np.random.default_rng(17)
    for (w, h) in SHAPES:
        img = _img(rng, w, h, 1)
        src = _dev(ctx, img)
        for block, bias in ((3, 0), (11, 2.5), (151, -4)):
            if (w, h) == (1920, 1080) and block == 151:
                continue
            exp = oracle.adaptive_threshold_mean(img, 255, False, block, bias)
            exp_inv = oracle.adaptive_threshold_mean(img, 255, True, block, bias)
            out = color.adaptive_threshold_mean(src, block, bias)
            inv = color.adaptive_threshold_mean_inv(src, block, bias)
            _resident(src, out, inv)
            assert out.binary and inv.binary
            assert np.array_equal(np.asarray(out), exp) and np.array_equal(np.asarray(inv), exp_inv), (w, h, block, bias)
            fo = cv2_facade.adaptiveThreshold(src, 200, cv2_facade.ADAPTIVE_THRESH_MEAN_C, cv2_facade.THRESH_BINARY, block, bias)
            _resident(src, fo)
            assert np.array_equal(np.asarray(fo), oracle.adaptive_threshold_mean(img, 200, False, block, bias))
            if (w, h) in SMALL:
                host = color.adaptive_threshold_mean(img, block, bias)
                assert type(host) is np.ndarray and np.array_equal(host, exp)
                host = cv2_facade.adaptiveThreshold(img, 255, cv2_facade.ADAPTIVE_THRESH_MEAN_C, cv2_facade.THRESH_BINARY_INV, block, bias)
                assert type(host) is np.ndarray and np.array_equal(host, exp_inv)
    img = _img(rng, 20, 10, 1)
    for s in (img, _dev(ctx, img)):
        with pytest.raises(vp.VpError):
            color.adaptive_threshold_mean(s, 153)
        with pytest.raises(cv2_facade.error):
            cv2_facade.adaptiveThreshold(s, 255, cv2_facade.ADAPTIVE_THRESH_MEAN_C, cv2_facade.THRESH_BINARY, 4, 0)


# ---- simple_canny, labelling ----------------------------------------------------------------------------------------------------------
def test_simple_canny_reads_a_histogram_not_the_image(vp, oracle):
    from vision.utils import feature
    ctx = vp.default_context()
    for (w, h) in ((67, 45), (640, 360), (1920, 1080)):
        gray, bgr = _device_gray(ctx, w, h)
        g = oracle.bgr2gray(bgr)
        for use_mean in (False, True):
            for sigma in (0.33, 0.1):
                mid = np.mean(g) if use_mean else np.median(g)
                lower, upper = int(max(0, (1.0 - sigma) * mid)), int(min(255, (1.0 + sigma) * mid))
                out = feature.simple_canny(gray, sigma, use_mean)
                _resident(gray, out)
                assert np.array_equal(np.asarray(out), oracle.canny(g, lower, upper)), (w, h, use_mean, sigma)
        hist = feature.device_histogram(gray)
        assert np.array_equal(hist, np.bincount(g.ravel(), minlength=256))
        _resident(gray)
    # multi-channel: the statistic is over all bytes, as numpy's
    bgr = F.s1_buoy(4, 640, 360)
    src = _dev(ctx, bgr)
    for use_mean in (False, True):
        mid = np.mean(bgr) if use_mean else np.median(bgr)
        out = feature.simple_canny(src, 0.33, use_mean)
        _resident(src, out)
        assert np.array_equal(np.asarray(out), oracle.canny(bgr, int(max(0, 0.67 * mid)), int(min(255, 1.33 * mid))))
    host = feature.simple_canny(bgr)
    assert type(host) is np.ndarray


def test_connected_components_dev_equals_the_oracle(vp, oracle):
    from vision import cv2_facade
    from vision.utils import color, feature
    from vision.devmat import DeviceMat
    ctx = vp.default_context()
    rng = np.random.default_rng(18)
    for (w, h) in SHAPES:
        mask = F.random_mask(rng, h, w, 0.5) if min(w, h) > 1 else (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
        for numbering in (2, 1):
            rn, rl, rs, rc = oracle.ccl(mask, numbering)
            src = _dev(ctx, mask)
            n, labels, stats, cent = feature.connected_components(src, numbering, max_labels=max(rn, 1))
            _resident(src, labels)
            assert n == rn and np.array_equal(stats, rs) and _same(cent, rc), (w, h, numbering)
            assert labels.dtype == np.int32 and np.array_equal(np.asarray(labels), rl), (w, h, numbering)
            n, labels, stats, cent = feature.connected_components(src, numbering, max_labels=max(rn, 1), want_labels=False)
            _resident(src)
            assert labels is None and n == rn and np.array_equal(stats, rs) and _same(cent, rc)
        hn, hl, hs, hc = feature.connected_components(mask, 2, max_labels=max(rn, 1))
        assert type(hl) is np.ndarray and hn == oracle.ccl(mask, 2)[0]
    # a mask that still owns the bit plane range_threshold made with it: labelled from the plane
    gray, bgr = _device_gray(ctx, 640, 360)
    th = color.range_threshold(gray, 90, 255)
    assert th._bits is not None
    exp_mask = oracle.inrange(oracle.bgr2gray(bgr), 90, 255)
    rn, rl, rs, rc = oracle.ccl(exp_mask, 2)
    calls = []
    L = vp.lib()
    real = L.vp_ccl_bits_dev

    class Spy:
        def __getattr__(self, name):
            if name == "vp_ccl_bits_dev":
                def f(*a):
                    calls.append(name)
                    return real(*a)
                return f
            return getattr(L, name)
    lib_fn = vp.lib
    vp.lib = lambda: Spy()
    try:
        n, labels, stats, cent = feature.connected_components(th, max_labels=max(rn, 1), want_labels=False)
    finally:
        vp.lib = lib_fn
    assert calls == ["vp_ccl_bits_dev"]
    _resident(gray, th)
    assert labels is None and n == rn and np.array_equal(stats, rs) and _same(cent, rc)
    n, labels, stats, cent = cv2_facade.connectedComponentsWithStats(th)
    _resident(th, labels)
    assert n == rn and np.array_equal(np.asarray(labels), rl) and np.array_equal(stats, rs)
    with pytest.raises(TypeError):
        feature.connected_components(DeviceMat.from_host(ctx, np.zeros((4, 4), np.float32)))


# ---- residency and a whole body --------------------------------------------------------------------------------------------------------
def test_operators_leave_device_images_on_the_device(vp, oracle):
    """On an image a device operator produced: after each of the operators neither the input nor the result has a host copy, and the
    result equals the expectation once looked at.  (Before these entries existed every one of them materialised its input.)"""
    from vision import cv2_facade
    from vision.utils import color, feature, transform
    ctx = vp.default_context()
    w, h = 640, 360
    gray, bgr = _device_gray(ctx, w, h)
    g = oracle.bgr2gray(bgr)
    frame = _dev(ctx, bgr)
    lab = color.bgr_to_lab(frame)[0]
    olab = oracle.bgr2lab(bgr)
    _resident(frame, lab)
    Mr = oracle.rotation_matrix_2d((w / 2, h / 2), 12.0, 1.0)
    ops = [
        ("simple_gaussian_blur", lambda: transform.simple_gaussian_blur(lab, 5, 0), lab, lambda: oracle.gaussian_blur(olab, (5, 5))),
        ("GaussianBlur gray", lambda: cv2_facade.GaussianBlur(gray, (7, 7), 1.5), gray, lambda: oracle.gaussian_blur(g, (7, 7), 1.5)),
        ("resize", lambda: transform.resize(lab, 320, 200), lab, lambda: RR.resize(olab, dsize=(320, 200))),
        ("rotate", lambda: transform.rotate(lab, 12.0), lab, lambda: oracle.warp_affine(olab, Mr, (w, h), border="replicate")),
        ("translate", lambda: transform.translate(gray, 5, 7), gray, lambda: oracle.warp_affine(g, np.float32([[1, 0, 5], [0, 1, 7]]), (w, h))),
        ("max_threshold", lambda: color.max_threshold(gray, 120), gray, lambda: _np_threshold(g, 120, 0, 2)),
        ("above_threshold", lambda: color.above_threshold(gray, 120), gray, lambda: _np_threshold(g, 120, 0, 3)),
        ("below_threshold", lambda: color.below_threshold(gray, 120), gray, lambda: _np_threshold(g, 120, 0, 4)),
        ("cv2.threshold", lambda: cv2_facade.threshold(gray, 120, 255, 0)[1], gray, lambda: _np_threshold(g, 120, 255, 0)),
        ("otsu_threshold", lambda: color.otsu_threshold(gray)[1], gray, lambda: np.where(g > _otsu_expectation(g), 255, 0).astype(np.uint8)),
        ("adaptive_threshold_mean", lambda: color.adaptive_threshold_mean(gray, 15, 2), gray, lambda: oracle.adaptive_threshold_mean(g, 255, False, 15, 2)),
        ("adaptiveThreshold", lambda: cv2_facade.adaptiveThreshold(gray, 255, 0, 1, 15, 2), gray, lambda: oracle.adaptive_threshold_mean(g, 255, True, 15, 2)),
    ]
    for name, run, src, expect in ops:
        out = run()
        assert type(out).__name__ == "DeviceMat", name
        assert src._host is None, f"{name} downloaded its input"
        assert out._host is None, f"{name} downloaded its result"
        assert np.array_equal(np.asarray(out), expect()), name
    edges = feature.simple_canny(gray)
    assert gray._host is None, "simple_canny downloaded its input"
    mid = np.median(g)
    assert np.array_equal(np.asarray(edges), oracle.canny(g, int(max(0, 0.67 * mid)), int(min(255, 1.33 * mid))))
    th = color.range_threshold(gray, 100, 255)
    n, labels, stats, cent = feature.connected_components(th, want_labels=False)
    assert th._host is None and gray._host is None, "connected_components downloaded its input"
    rn, _, rs, rc = oracle.ccl(oracle.inrange(g, 100, 255), 2, want_labels=False)
    assert n == rn and np.array_equal(stats, rs[:len(stats)]) and _same(cent, rc[:len(cent)])


def test_a_whole_body_stays_in_hbm(vp, oracle):
    """blur -> bgr_to_lab -> range_threshold -> open -> close -> outer_contours and -> connected_components, the frame given as a
    DeviceMat: equals the oracle's chain on the blurred frame, and no image of it has a host copy afterwards."""
    from vision.utils import color, feature, transform
    ctx = vp.default_context()
    for (w, h) in ((640, 360), (1920, 1080)):
        bgr = F.s1_buoy(5, w, h)
        frame = _dev(ctx, bgr)
        blurred = transform.simple_gaussian_blur(frame, 5, 0)
        lab, planes = color.bgr_to_lab(blurred)
        th = color.range_threshold(lab, (0, 150, 0), (255, 255, 255))
        opened = transform.morph_remove_noise(th, transform.rect_kernel(5))
        cleaned = transform.morph_close_holes(opened, transform.rect_kernel(5))
        contours = feature.outer_contours(cleaned)
        n, labels, stats, cent = feature.connected_components(cleaned)
        images = (frame, blurred, lab) + tuple(planes) + (th, opened, cleaned, labels)
        for m in images:
            assert m._host is None, "an image of the body was downloaded"
        ob = oracle.gaussian_blur(bgr, (5, 5))
        ref = oracle.chain(ob, oracle.MODE_LAB, (0, 150, 0), (255, 255, 255), [oracle.OPEN, oracle.CLOSE], 5, 5, 2, 4096)
        exp_c = oracle.find_contours(ref["cleaned"], oracle.RETR_EXTERNAL, oracle.CHAIN_APPROX_SIMPLE)
        assert len(contours) == len(exp_c) and all(np.array_equal(a, b) for a, b in zip(contours, exp_c))
        assert n == ref["nlabels"] and np.array_equal(stats, ref["stats"]) and _same(cent, ref["centroids"])
        assert np.array_equal(np.asarray(blurred), ob)
        assert np.array_equal(np.asarray(th), ref["threshed"]) and np.array_equal(np.asarray(cleaned), ref["cleaned"])
        assert np.array_equal(np.asarray(labels), ref["labels"])
