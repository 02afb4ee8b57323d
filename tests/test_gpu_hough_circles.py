"""GPU suite: cv2.HoughCircles (HOUGH_GRADIENT) on the MI355X (csrc/vp_hough_circles.hip) equals the statement of the tests
(hough_circles_restate.py) bit for bit - the circle array, its order and None-ness - through the host and device entries, the mirror's
hough_circles and the facade, with the radius histograms in LDS and in the workspace."""
import numpy as np
import pytest

import frames as F
import hough_circles_restate as HC
from test_hough_circles_statement import discs

pytestmark = pytest.mark.gpu


def _same(got, exp, what=""):
    if exp is None:
        assert got is None, f"{what}: expected no circle, got {0 if got is None else got.shape[1]}"
        return
    assert got is not None, f"{what}: expected {exp.shape[1]} circles, got None"
    assert got.dtype == np.float32 and got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.any(got.view(np.uint32) != exp.view(np.uint32), axis=2)[0]
    assert not bad.any(), f"{what}: circles differ (first at {int(np.argmax(bad))}: {got[0, np.argmax(bad)]} vs {exp[0, np.argmax(bad)]})"


def _host_call(vp, img, dp, md, p1=100, p2=100, rmin=0, rmax=0, cap=1 << 16):
    ctx = vp.default_context()
    out = np.full((max(cap, 1), 3), -1.0, np.float32)
    n = vp.C.c_int(-1)
    img = np.ascontiguousarray(img)
    vp.check(vp.lib().vp_hough_circles_u8(ctx.handle, vp.ptr(img), img.shape[1], img.shape[0], float(dp), float(md), float(p1), float(p2),
                                          int(rmin), int(rmax), vp.ptr(out), cap, vp.C.byref(n)), ctx.handle)
    return n.value, out


def _gray(img):
    return np.ascontiguousarray(img[:, :, 1])


def test_tiny_and_odd_shapes(vp):
    from vision import cv2_facade
    rng = np.random.default_rng(5)
    for h, w in ((1, 1), (1, 17), (23, 1), (3, 5), (31, 29), (333, 101)):
        for kind in ("noise", "flat"):
            img = rng.integers(0, 256, (h, w)).astype(np.uint8) if kind == "noise" else np.full((h, w), 77, np.uint8)
            for p2 in (1, 5, 100):
                _same(cv2_facade.HoughCircles(img, cv2_facade.HOUGH_GRADIENT, 1, 3, None, 60, p2), HC.hough_circles(img, 1, 3, 60, p2),
                      f"{h}x{w} {kind} p2={p2}")


@pytest.mark.parametrize("dp", [0.5, 1, 1.5, 2])
def test_buoy_frames_parameters(vp, dp):
    from vision.utils.feature import hough_circles
    for i in range(2):
        g = _gray(F.s1_buoy(i, 320, 240))
        for md, p1, p2, rmin, rmax in ((20, 100, 20, 0, 0), (1, 100, 12, 5, 60), (200, 60, 15, 0, 90), (20, 100, 20, 30, 30),
                                       (20, 100, 20, 40, 10), (20, 100, 10000, 0, 0), (5.5, 150.5, 9.5, 3, 70)):
            _same(hough_circles(g, dp, md, p1, p2, rmin, rmax), HC.hough_circles(g, dp, md, p1, p2, rmin, rmax),
                  f"frame {i} dp={dp} md={md} p1={p1} p2={p2} r={rmin}..{rmax}")


def test_discs_and_bins(vp):
    from vision.utils.feature import hough_circles
    img = discs(1, 240, 320, ((80, 70, 30), (220, 150, 45), (270, 50, 18)))
    for dp in (1, 1.5, 2):
        exp = HC.hough_circles(img, dp, 20, 100, 20, 10, 80)
        assert exp is not None
        _same(hough_circles(img, dp, 20, 100, 20, 10, 80), exp, f"discs dp={dp}")
    for i in range(2):
        g = _gray(F.s2_bins(i, 640, 360))
        for args in ((1, 20, 100, 30, 0, 120), (2, 10, 80, 15, 5, 100)):
            _same(hough_circles(g, *args), HC.hough_circles(g, *args), f"bins {i} {args}")


def test_noise_with_thousands_of_centres(vp):
    """A low param2 on noise: thousands of accumulator centres, so the key sort's merge passes run, and many supported circles."""
    from vision.utils.feature import hough_circles
    g = _gray(F.s3_noise(0, 320, 240))
    a = HC.arguments(g.shape, 1, 2, 100, 2, 0, 12)
    from oracle import oracle as orc
    acc, _ = HC.accumulator(g, a, orc.canny)
    ofs, _ = HC.centres(acc, a["acc_thresh"])
    assert len(ofs) > 2048, len(ofs)
    _same(hough_circles(g, 1, 2, 100, 2, 0, 12), HC.hough_circles(g, 1, 2, 100, 2, 0, 12), "noise p2=2")


@pytest.mark.parametrize("rmin,rmax", [(0, 0), (10, 120)])
def test_full_hd_buoy_frame(vp, rmin, rmax):
    """One 1080p buoy frame at the reference's defaults (canny_thresh = circle_thresh = 100, radii 0) and at a bounded radius range."""
    from vision.utils.feature import hough_circles
    g = _gray(F.s1_buoy(0))
    exp = HC.hough_circles(g, 1, 20, 100, 100, rmin, rmax)
    _same(hough_circles(g, 1, 20, 100, 100, rmin, rmax), exp, f"1080p r={rmin}..{rmax}")
    if rmax:
        g2 = _gray(F.s1_buoy(3))
        _same(hough_circles(g2, 2, 30, 100, 40, rmin, rmax), HC.hough_circles(g2, 2, 30, 100, 40, rmin, rmax), f"1080p dp=2 r={rmin}..{rmax}")


def test_global_histograms_equal_lds(vp):
    from vision.utils.feature import hough_circles
    ctx = vp.default_context()
    g = _gray(F.s1_buoy(1, 320, 240))
    cases = ((1, 10, 100, 12, 0, 0), (1.5, 5, 100, 8, 4, 70), (1, 2, 100, 2, 0, 12))
    exp = [HC.hough_circles(g, *c) for c in cases]
    try:
        ctx.set_option(vp.OPT_HOUGH_CIRCLES_LDS, 0)
        for c, e in zip(cases, exp):
            _same(hough_circles(g, *c), e, f"workspace histograms {c}")
    finally:
        ctx.set_option(vp.OPT_HOUGH_CIRCLES_LDS, 1)
    for c, e in zip(cases, exp):
        _same(hough_circles(g, *c), e, f"LDS histograms {c}")
    # more bins than LDS holds (a radius range of 8000 at dp = 1: 80 000 bins) take the workspace form on their own
    small = discs(2, 120, 160, ((60, 60, 25),))
    _same(hough_circles(small, 1, 10, 100, 20, 0, 8000), HC.hough_circles(small, 1, 10, 100, 20, 0, 8000), "80 000 bins")


def test_large_lds_histograms_with_centres(vp):
    """The reference's default maxRadius on a wide frame needs more than 16 384 bins: the radius stage then asks for 64-160 KiB of
    dynamic LDS.  Discs with circles in them at 20 000 bins, at exactly 160 KiB (40 960 bins) and one radius above it (40 970 bins,
    the workspace form on its own), each also through the forced workspace form."""
    from vision.utils.feature import hough_circles
    ctx = vp.default_context()
    img = discs(1, 240, 320, ((80, 70, 30), (220, 150, 45), (270, 50, 18)))
    for rmax in (2000, 4096, 4097):
        exp = HC.hough_circles(img, 1, 20, 100, 20, 0, rmax)
        assert exp is not None and exp.shape[1] >= 3, (rmax, exp)
        _same(hough_circles(img, 1, 20, 100, 20, 0, rmax), exp, f"maxRadius {rmax} ({rmax * 10} bins)")
        try:
            ctx.set_option(vp.OPT_HOUGH_CIRCLES_LDS, 0)
            _same(hough_circles(img, 1, 20, 100, 20, 0, rmax), exp, f"maxRadius {rmax}, workspace histograms")
        finally:
            ctx.set_option(vp.OPT_HOUGH_CIRCLES_LDS, 1)


def test_short_buffer_returns_true_count_and_calls_repeat(vp):
    g = _gray(F.s1_buoy(0, 320, 240))
    exp = HC.hough_circles(g, 1, 10, 100, 12)
    assert exp is not None and exp.shape[1] > 3
    n, full = _host_call(vp, g, 1, 10, 100, 12)
    assert n == exp.shape[1]
    _same(full[None, :n].copy(), exp, "full buffer")
    for cap in (0, 1, 3):
        n2, buf = _host_call(vp, g, 1, 10, 100, 12, cap=cap)
        assert n2 == n, (cap, n2, n)
        if cap:
            _same(buf[None, :cap].copy(), exp[:, :cap], f"cap {cap}")
            assert np.all(buf[cap:] == -1.0)
    n3, again = _host_call(vp, g, 1, 10, 100, 12)
    assert n3 == n and again.tobytes() == full.tobytes(), "two identical calls gave different bytes"


def test_device_entry_and_devmat(vp):
    import torch
    from vision.devmat import DeviceMat
    from vision.utils.feature import hough_circles
    g = _gray(F.s1_buoy(2, 320, 240))
    exp = HC.hough_circles(g, 1.5, 15, 90, 14, 2, 90)
    dm = DeviceMat.from_host(vp.default_context(), g)
    _same(hough_circles(dm, 1.5, 15, 90, 14, 2, 90), exp, "DeviceMat")
    pitched = np.zeros((240, 384), np.uint8)
    pitched[:, :320] = g
    dev = torch.from_numpy(pitched.ravel()).cuda()
    torch.cuda.synchronize()
    ctx = vp.default_context()
    out = np.empty((4096, 3), np.float32)
    n = vp.C.c_int(-1)
    vp.check(vp.lib().vp_hough_circles_dev(ctx.handle, dev.data_ptr(), 384, 320, 240, 1.5, 15.0, 90.0, 14.0, 2, 90, vp.ptr(out), 4096,
                                           vp.C.byref(n)), ctx.handle)
    _same(out[None, :n.value].copy() if n.value else None, exp, "pitched device image")


def test_facade_and_errors(vp):
    from vision import cv2_facade
    g = _gray(F.s1_buoy(1, 320, 240))
    _same(cv2_facade.HoughCircles(g, cv2_facade.HOUGH_GRADIENT, 1, 20, None, 100, 20, 0, 0), HC.hough_circles(g, 1, 20, 100, 20), "facade")
    _same(cv2_facade.HoughCircles(g[:, :, None], cv2_facade.HOUGH_GRADIENT, 2, 20, param2=15, minRadius=5, maxRadius=50),
          HC.hough_circles(g, 2, 20, 100, 15, 5, 50), "facade keywords")
    ctx = vp.default_context()
    out = np.empty((4, 3), np.float32)
    n = vp.C.c_int(-1)
    for dp, md, p1, p2, rmax, rc in ((0, 1, 1, 1, 0, -1), (1, 0, 1, 1, 0, -1), (1, 1, -1, 1, 0, -1), (1, 1, 1, 0, 0, -1), (1, 1, 1, 1, -1, -4)):
        got = vp.lib().vp_hough_circles_u8(ctx.handle, vp.ptr(g), 320, 240, float(dp), float(md), float(p1), float(p2), 0, rmax, vp.ptr(out), 4,
                                           vp.C.byref(n))
        assert got == rc, (dp, md, p1, p2, rmax, got)
