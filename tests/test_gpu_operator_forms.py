"""The two forms of every operator that goes through vision.utils.helpers.run_operator: a numpy image (libvp's host entry, numpy out)
and a DeviceMat (the device entry, a DeviceMat out).  Each form is compared, byte for byte, with the statement or the oracle that the
family's own GPU suite uses - never one form with the other.  The images are the smallest that exercise the fork rather than the
kernels: (7, 5), (9, 13, 3), (7, 5, 1) and a view with a column stride.  And one call of each device form queues as many kernels as it
did before the fork was written once."""
import functools

import numpy as np
import pytest

import box_pyr_restate as BR
import clahe_restate as CR
import deriv_restate as DR
import remap_restate as MR
import resize_restate as RR
from median_restate import majority_restate, median_restate

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _images():
    rng = np.random.default_rng(1905)
    wide = rng.integers(0, 256, (6, 10), dtype=np.uint8)
    imgs = {"grey": rng.integers(0, 256, (7, 5), dtype=np.uint8), "bgr": rng.integers(0, 256, (9, 13, 3), dtype=np.uint8),
            "one": rng.integers(0, 256, (7, 5, 1), dtype=np.uint8), "view": wide[:, ::2]}
    assert not imgs["view"].flags.c_contiguous
    for a in (wide, *imgs.values()):
        a.flags.writeable = False
    return imgs


GREY_ONLY = ("grey", "one", "view")
ALL = ("grey", "bgr", "one", "view")
PERSPECTIVE = np.array([[1.05, 0.08, -0.6], [-0.04, 0.97, 0.8], [0.003, -0.002, 1.0]])


def _maps(img):
    h, w = img.shape[:2]
    rng = np.random.default_rng(h * 100 + w)
    return (rng.random((6, 4), dtype=np.float32) * (w + 2) - 1).astype(np.float32), (rng.random((6, 4), dtype=np.float32) * (h + 2) - 1).astype(np.float32)


def _plane(img):
    return img[:, :, 0] if img.ndim == 3 and img.shape[2] == 1 else img


def _like(img, out):
    """the statement's result of the (h, w) plane under the shape the library gives for an (h, w, 1) source"""
    return out[:, :, None] if img.ndim == 3 and img.shape[2] == 1 else out


def _rotation(oracle, img):
    h, w = img.shape[:2]
    return oracle.rotation_matrix_2d((w / 2, h / 2), 10.0, 1.0)


# name -> (images, call(transform, facade, color, source), expectation(oracle, image)); a tuple or list of results is compared item by item
OPERATORS = {
    "simple_gaussian_blur": (ALL, lambda t, f, c, s: t.simple_gaussian_blur(s, 5, 0), lambda o, a: o.gaussian_blur(a, (5, 5), 0.0, 0.0)),
    "GaussianBlur": (ALL, lambda t, f, c, s: f.GaussianBlur(s, (3, 5), 1.2), lambda o, a: o.gaussian_blur(a, (3, 5), 1.2, 0.0)),
    "resize": (ALL, lambda t, f, c, s: t.resize(s, 8, 6), lambda o, a: _like(a, RR.resize(_plane(a), dsize=(8, 6)))),
    "resize scaled": (ALL, lambda t, f, c, s: f.resize(s, None, fx=1.4, fy=0.8), lambda o, a: _like(a, RR.resize(_plane(a), fx=1.4, fy=0.8))),
    "rotate": (ALL, lambda t, f, c, s: t.rotate(s, 10.0),
               lambda o, a: o.warp_affine(a, _rotation(o, a), (a.shape[1], a.shape[0]), border="replicate")),
    "translate": (ALL, lambda t, f, c, s: t.translate(s, 1, 2), lambda o, a: o.warp_affine(a, np.float32([[1, 0, 1], [0, 1, 2]]), (a.shape[1], a.shape[0]))),
    "median_blur": (ALL, lambda t, f, c, s: t.median_blur(s, 3), lambda o, a: _like(a, median_restate(_plane(a), 3))),
    "sobel": (ALL, lambda t, f, c, s: t.sobel(s, 1, 0), lambda o, a: _like(a, DR.sobel_restate(_plane(a), DR.CV_16S, 1, 0))),
    "Scharr": (ALL, lambda t, f, c, s: f.Scharr(s, f.CV_32F, 0, 1), lambda o, a: _like(a, DR.scharr_restate(_plane(a), DR.CV_32F, 0, 1))),
    "laplacian": (ALL, lambda t, f, c, s: t.laplacian(s, 3), lambda o, a: _like(a, DR.laplacian_restate(_plane(a), DR.CV_16S, 3))),
    "spatial_gradient": (GREY_ONLY, lambda t, f, c, s: t.spatial_gradient(s), lambda o, a: DR.spatial_gradient_restate(_plane(a))),
    "convert_scale_abs": (ALL, lambda t, f, c, s: t.convert_scale_abs(s), lambda o, a: DR.convert_scale_abs_restate(a)),
    "box_filter": (ALL, lambda t, f, c, s: t.box_filter(s, 3), lambda o, a: _like(a, BR.box_filter_restate(_plane(a), -1, 3, 3))),
    "boxFilter sums": (ALL, lambda t, f, c, s: f.boxFilter(s, f.CV_32S, (2, 3), normalize=False),
                       lambda o, a: _like(a, BR.box_filter_restate(_plane(a), BR.CV_32S, 2, 3, False))),
    "pyr_down": (ALL, lambda t, f, c, s: t.pyr_down(s), lambda o, a: _like(a, BR.pyr_down_restate(_plane(a)))),
    "pyr_up": (ALL, lambda t, f, c, s: t.pyr_up(s), lambda o, a: _like(a, BR.pyr_up_restate(_plane(a)))),
    # (without the (h, w, 1) image: its numpy form uploads through device_image, which drops the axis, and its DeviceMat form keeps it)
    "build_pyramid": (("grey", "bgr", "view"), lambda t, f, c, s: t.build_pyramid(s, 2),
                      lambda o, a: [np.ascontiguousarray(a), _like(a, BR.pyr_down_restate(_plane(a))), _like(a, BR.pyr_down_restate(BR.pyr_down_restate(_plane(a))))]),
    "integral": (ALL, lambda t, f, c, s: t.integral(s), lambda o, a: _like(a, BR.integral_restate(_plane(a)))),
    "equalize_hist": (GREY_ONLY, lambda t, f, c, s: c.equalize_hist(s), lambda o, a: CR.equalize_hist(_plane(a))),
    "clahe": (GREY_ONLY, lambda t, f, c, s: c.clahe(s, 2.0, (2, 2)), lambda o, a: CR.clahe(_plane(a), 2.0, (2, 2))),
    "remap": (ALL, lambda t, f, c, s: t.remap(s, *_maps(s)), lambda o, a: _like(a, MR.remap_restate(_plane(a), *_maps(a)))),
    "warp_perspective": (ALL, lambda t, f, c, s: t.warp_perspective(s, PERSPECTIVE, 6, 8),
                         lambda o, a: _like(a, MR.warp_perspective_restate(_plane(a), PERSPECTIVE, (6, 8)))),
}
SIGNED = DR.sobel_restate(np.arange(35, dtype=np.uint8).reshape(7, 5) * 7, DR.CV_16S, 1, 0)       # convert_scale_abs also takes int16


@functools.lru_cache(maxsize=None)
def _expected(oracle, name, key):
    out = OPERATORS[name][2](oracle, _images()[key])
    return out if isinstance(out, (tuple, list)) else (out,)


def _same(got, exp):
    return got.dtype == exp.dtype and tuple(got.shape) == tuple(exp.shape) and np.asarray(got).tobytes() == np.ascontiguousarray(exp).tobytes()


@pytest.mark.parametrize("name", sorted(OPERATORS))
def test_both_forms_against_the_statement(vp, oracle, name):
    from vision import cv2_facade as f
    from vision.devmat import DeviceMat
    from vision.utils import color as c
    from vision.utils import transform as t
    ctx = vp.default_context()
    keys, call, _ = OPERATORS[name]
    for key in keys:
        img = _images()[key]
        exp = _expected(oracle, name, key)
        host = call(t, f, c, img)
        host = host if isinstance(host, (tuple, list)) else (host,)
        assert len(host) == len(exp) and all(type(h) is np.ndarray and _same(h, e) for h, e in zip(host, exp)), (name, key, "numpy form")
        src = DeviceMat.from_host(ctx, img)
        dev = call(t, f, c, src)
        dev = dev if isinstance(dev, (tuple, list)) else (dev,)
        assert len(dev) == len(exp) and all(isinstance(d, DeviceMat) and not d.binary for d in dev), (name, key, "DeviceMat form")
        assert src._host is None and all(d._host is None for d in dev if d is not src), (name, key, "a host copy was made")
        assert all(_same(d, e) for d, e in zip(dev, exp)), (name, key, "DeviceMat form")


def test_convert_scale_abs_of_a_signed_image(vp):
    from vision.devmat import DeviceMat
    from vision.utils import transform as t
    exp = DR.convert_scale_abs_restate(SIGNED)
    host = t.convert_scale_abs(SIGNED)
    assert type(host) is np.ndarray and _same(host, exp)
    dev = t.convert_scale_abs(DeviceMat.from_host(vp.default_context(), SIGNED))
    assert isinstance(dev, DeviceMat) and not dev.binary and _same(dev, exp)


def test_median_blur_of_a_mask_keeps_the_flag_and_brings_a_bit_plane(vp):
    """range_threshold -> median_blur as tests/test_gpu_median.py has it: the mask comes with its bit plane, and so does the result"""
    from vision.devmat import DeviceMat
    from vision.utils import transform as t
    from vision.utils.color import range_threshold
    ctx = vp.default_context()
    rng = np.random.default_rng(64)
    grey = np.where(rng.random((9, 64)) < 0.4, 200, 10).astype(np.uint8)
    host_mask = np.where(grey >= 150, 255, 0).astype(np.uint8)
    mask = range_threshold(DeviceMat.from_host(ctx, grey), 150, 255)
    assert mask.binary
    out = t.median_blur(mask, 3)
    assert mask._bits is not None, "the 64-wide mask came without its bit plane"
    assert isinstance(out, DeviceMat) and out.binary and out._bits is not None
    assert _same(out, majority_restate(host_mask, 3))
    narrow = t.median_blur(range_threshold(DeviceMat.from_host(ctx, np.ascontiguousarray(grey[:, :40])), 150, 255), 3)   # no whole words: a mask, no plane
    assert narrow.binary and narrow._bits is None and _same(narrow, majority_restate(np.ascontiguousarray(host_mask[:, :40]), 3))
    plain = t.median_blur(DeviceMat.from_host(ctx, host_mask), 3)                         # not known to be a mask: no flag, no plane
    assert not plain.binary and plain._bits is None and _same(plain, median_restate(host_mask, 3))
    host = t.median_blur(host_mask, 3)
    assert type(host) is np.ndarray and _same(host, median_restate(host_mask, 3))


# Kernels queued by one call of the device form on the (9, 13, 3) image (the (7, 5) one for the single-channel operators), counted with
# ctx.profile_begin / profile_end on commit 1194311, the parent of the commit that wrote the fork once.
# (convert_scale_abs: its kernel is not among those the profile names, so the count is 0 on both sides of the change.)
LAUNCHES = {"GaussianBlur": 1, "Scharr": 1, "boxFilter sums": 1, "box_filter": 1, "build_pyramid": 2, "clahe": 1, "convert_scale_abs": 0, "equalize_hist": 2,
            "integral": 1, "laplacian": 1, "median_blur": 1, "pyr_down": 1, "pyr_up": 1, "remap": 1, "resize": 1, "resize scaled": 1, "rotate": 1,
            "simple_gaussian_blur": 1, "sobel": 1, "spatial_gradient": 1, "translate": 1, "warp_perspective": 1}


@pytest.mark.parametrize("name", sorted(OPERATORS))
def test_device_form_queues_the_kernels_it_did(vp, name):
    assert launches(vp, name) == LAUNCHES[name]


def launches(vp, name):
    """kernels queued by one call of the operator's device form"""
    from vision import cv2_facade as f
    from vision.devmat import DeviceMat
    from vision.utils import color as c
    from vision.utils import transform as t
    ctx = vp.default_context()
    keys, call, _ = OPERATORS[name]
    src = DeviceMat.from_host(ctx, _images()["bgr" if "bgr" in keys else "grey"])
    call(t, f, c, src)                                   # (tables that an operator builds once are built now)
    ctx.synchronize()
    ctx.profile_begin(64)
    out = call(t, f, c, src)
    prof = ctx.profile_end()
    del out
    return sum(v[1] for v in prof.values())
