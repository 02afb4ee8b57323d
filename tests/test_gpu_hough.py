"""GPU suite: cv2.HoughLines on the MI355X (csrc/vp_hough.hip) equals the statement of the tests (hough_restate.py) bit for bit - the line
array, its order and None-ness - through the host, device and batch entries, the mirror (find_lines) and the facade (HoughLines)."""
import numpy as np
import pytest

import frames as F
import hough_restate as HR

pytestmark = pytest.mark.gpu

STEP = np.pi / 180


def _same(got, exp, what=""):
    if exp is None:
        assert got is None, f"{what}: expected no line, got {0 if got is None else len(got)}"
        return
    assert got is not None, f"{what}: expected {len(exp)} lines, got None"
    assert got.dtype == np.float32 and got.shape == exp.shape, (what, got.shape, exp.shape)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), f"{what}: lines differ (first at {np.argmax(np.any(got != exp, axis=(1, 2)))})"


def _noise(seed, h, w, p):
    return ((np.random.default_rng(seed).random((h, w)) < p) * 255).astype(np.uint8)


def _host_call(vp, img, rho, theta, thr, lo=0.0, hi=np.pi, cap=1 << 20):
    ctx = vp.default_context()
    out = np.empty((max(cap, 1), 1, 2), np.float32)
    n = vp.C.c_int(-1)
    img = np.ascontiguousarray(img)
    vp.check(vp.lib().vp_hough_lines_u8(ctx.handle, vp.ptr(img), img.shape[1], img.shape[0], float(rho), float(theta), int(thr), float(lo),
                                        float(hi), vp.ptr(out), cap, vp.C.byref(n)), ctx.handle)
    return n.value, out


def test_tiny_and_odd_shapes(vp):
    from vision import cv2_facade
    rng = np.random.default_rng(5)
    for h, w in ((1, 1), (1, 17), (23, 1), (1, 300), (257, 1), (3, 5), (31, 29), (127, 255), (333, 101)):
        for p in (0.0, 0.3, 1.0):
            img = ((rng.random((h, w)) < p) * 255).astype(np.uint8)
            for thr in (0, 1, 5):
                _same(cv2_facade.HoughLines(img, 1, STEP, thr), HR.hough_lines(img, 1, STEP, thr), f"{h}x{w} p={p} thr={thr}")


def test_canny_of_the_frame_families(vp):
    from vision.utils.feature import canny, hough_lines
    cases = [F.s1_buoy(0, 640, 360), F.s2_bins(1, 640, 360), F.s3_noise(2, 320, 240), F.s4_flat(90, 200, 100)]
    for k, img in enumerate(cases):
        gray = np.ascontiguousarray(img[:, :, 1])
        edges = canny(gray, 50, 150)
        assert isinstance(edges, np.ndarray)
        for thr in (20, 60, 150):
            _same(hough_lines(edges, 1, STEP, thr), HR.hough_lines(edges, 1, STEP, thr), f"family {k} thr={thr}")


@pytest.mark.parametrize("w,h", [(1920, 1080), (3840, 2160)])
def test_large_edge_images(vp, w, h):
    from vision.utils.feature import canny, hough_lines
    img = F.s2_bins(4, w, h)
    edges = canny(np.ascontiguousarray(img[:, :, 2]), 40, 120)
    for thr in (100, 300):
        _same(hough_lines(edges, 1, STEP, thr), HR.hough_lines(edges, 1, STEP, thr), f"{w}x{h} thr={thr}")


@pytest.mark.parametrize("p,thr", [(0.02, 2), (0.10, 8), (0.50, 60)])
def test_noise_forces_the_multi_block_sort(vp, p, thr):
    img = _noise(int(p * 100), 360, 480, p)
    exp = HR.hough_lines(img, 1, STEP, thr)
    assert exp is not None and len(exp) > 4 * 2048, len(exp)      # several sorted runs to merge
    n, out = _host_call(vp, img, 1, STEP, thr)
    assert n == len(exp)
    _same(out[:n], exp, f"noise {p}")


def test_noise_on_the_one_block_sort(vp):
    img = _noise(9, 360, 480, 0.02)
    exp = HR.hough_lines(img, 1, STEP, 14)
    assert exp is not None and 0 < len(exp) <= 2048, len(exp)
    n, out = _host_call(vp, img, 1, STEP, 14)
    _same(out[:n], exp, "one block")


@pytest.mark.parametrize("rho,theta,lo,hi", [(0.5, STEP, 0.0, np.pi), (2, np.pi / 90, 0.0, np.pi), (1, np.pi / 360, 0.0, np.pi), (1.5, 0.3, 0.0, np.pi),
                                             (1, 1.0, 0.0, np.pi), (1, STEP, np.pi / 4, 3 * np.pi / 4), (0.7, 0.01, -1.0, 2.5)])
def test_resolutions_and_angle_ranges(vp, rho, theta, lo, hi):
    from vision import cv2_facade
    gray = np.ascontiguousarray(F.s1_buoy(7, 400, 300)[:, :, 2])
    edges = cv2_facade.Canny(gray, 40, 120)
    for thr in (10, 40):
        _same(cv2_facade.HoughLines(edges, rho, theta, thr, None, 0, 0, lo, hi), HR.hough_lines(edges, rho, theta, thr, lo, hi),
              f"rho={rho} theta={theta} [{lo}, {hi}] thr={thr}")


def test_lds_and_global_voting_agree(vp):
    from vision.utils.feature import hough_lines
    ctx = vp.default_context()
    img = _noise(11, 300, 400, 0.05)
    exp = HR.hough_lines(img, 1, STEP, 20)
    try:
        ctx.set_option(vp.OPT_HOUGH_LDS, 0)
        _same(hough_lines(img, 1, STEP, 20), exp, "global atomics")
    finally:
        ctx.set_option(vp.OPT_HOUGH_LDS, 1)
    _same(hough_lines(img, 1, STEP, 20), exp, "LDS rows")
    # rows wider than the LDS budget (4K at rho = 0.5: 24 002 cells) take the global form on their own
    big = np.zeros((2160, 3840), np.uint8)
    big[1000, 100:3000] = 255
    big[:, 2500] = 255
    big[np.arange(2000), np.arange(2000) + 500] = 255
    _same(hough_lines(big, 0.5, STEP, 500), HR.hough_lines(big, 0.5, STEP, 500), "4K rho 0.5")


def test_small_capacity_gives_a_prefix_and_the_true_count(vp):
    img = _noise(12, 200, 300, 0.1)
    exp = HR.hough_lines(img, 1, STEP, 5)
    assert len(exp) > 100
    for cap in (0, 1, 7, 100):
        n, out = _host_call(vp, img, 1, STEP, 5, cap=cap)
        assert n == len(exp)
        if cap:
            _same(out[:cap], exp[:cap], f"cap {cap}")
    # nothing is written past the capacity
    ctx = vp.default_context()
    buf = np.full((64, 1, 2), -7.0, np.float32)
    n = vp.C.c_int(-1)
    vp.check(vp.lib().vp_hough_lines_u8(ctx.handle, vp.ptr(img), 300, 200, 1.0, STEP, 5, 0.0, np.pi, vp.ptr(buf), 10, vp.C.byref(n)), ctx.handle)
    assert n.value == len(exp) and np.all(buf[10:] == -7.0)
    _same(buf[:10].copy(), exp[:10], "cap 10")


def test_batch_equals_per_frame_calls(vp):
    import torch
    from vision.utils.feature import hough_lines
    frames = [_noise(20 + i, 240, 320, p) for i, p in enumerate((0.0, 0.01, 0.03, 0.2))]
    gray = np.ascontiguousarray(F.s2_bins(3, 320, 240)[:, :, 1])
    from vision import cv2_facade
    frames.append(cv2_facade.Canny(gray, 30, 90))
    frames.append(np.zeros((240, 320), np.uint8))
    frames[-1][100, :] = 255
    stack = np.stack(frames)
    flat = np.zeros(len(frames) * (240 * 384 + 4096), np.uint8)
    for i in range(len(frames)):
        o = i * (240 * 384 + 4096)
        flat[o:o + 240 * 384].reshape(240, 384)[:, :320] = stack[i]     # row stride 384, frame stride 240 * 384 + 4096
    dev = torch.from_numpy(flat).cuda()
    torch.cuda.synchronize()
    ctx = vp.default_context()
    for thr, cap in ((10, 4096), (40, 50)):
        out = np.full((len(frames), cap, 1, 2), -1.0, np.float32)
        counts = np.full(len(frames), -1, np.int32)
        vp.check(vp.lib().vp_hough_lines_batch_dev(ctx.handle, dev.data_ptr(), 384, 240 * 384 + 4096, len(frames), 320, 240, 1.0, STEP, thr, 0.0,
                                                   np.pi, vp.ptr(out), cap, vp.ptr(counts)), ctx.handle)
        for i, fr in enumerate(frames):
            exp = HR.hough_lines(fr, 1, STEP, thr)
            single = hough_lines(fr, 1, STEP, thr)
            _same(single, exp, f"frame {i} single")
            assert counts[i] == (0 if exp is None else len(exp)), (i, counts[i])
            k = min(cap, counts[i])
            _same(out[i, :k].copy() if k else None, None if exp is None else exp[:k], f"frame {i} batch thr={thr}")


def test_find_lines_on_a_device_canny_stays_on_the_device(vp):
    from vision.devmat import DeviceMat
    from vision.utils.color import bgr_to_gray
    from vision.utils.feature import canny, find_lines, line_polar_to_cartesian
    img = F.s2_bins(5, 640, 360)
    gray, _ = bgr_to_gray(DeviceMat.from_host(vp.default_context(), img))
    assert isinstance(gray, DeviceMat)
    edges = canny(gray, 40, 120)
    assert isinstance(edges, DeviceMat)
    cart, polar = find_lines(edges, 1, STEP, 60)
    assert edges._host is None and gray._host is None, "the edge image was downloaded although only find_lines read it"
    host_edges = np.asarray(edges)
    from vision import cv2_facade
    assert np.array_equal(host_edges, cv2_facade.Canny(np.asarray(gray), 40, 120))
    exp = HR.hough_lines(host_edges, 1, STEP, 60)
    assert exp is not None and len(polar) == len(exp) == len(cart)
    for (r, t), e, c in zip(polar, exp, cart):
        assert type(r) is np.float32 and type(t) is np.float32
        assert r.view(np.uint32) == e[0, 0].view(np.uint32) and t.view(np.uint32) == e[0, 1].view(np.uint32)
        assert c == line_polar_to_cartesian(e[0, 0], e[0, 1])
    assert find_lines(np.zeros((50, 60), np.uint8), 1, STEP, 1) == ([], [])


def test_invalid_arguments_are_errors(vp):
    from vision.utils.feature import hough_lines
    ctx = vp.default_context()
    img = np.zeros((40, 50), np.uint8)
    img[20, :] = 255
    out = np.zeros((8, 1, 2), np.float32)
    n = vp.C.c_int(-1)
    L = vp.lib()
    for rho, theta, lo, hi in ((0, STEP, 0, np.pi), (-1, STEP, 0, np.pi), (1, 0, 0, np.pi), (1, -0.1, 0, np.pi), (1, STEP, 1.0, 0.5),
                               (float("nan"), STEP, 0, np.pi), (1, STEP, 0, float("inf"))):
        assert L.vp_hough_lines_u8(ctx.handle, vp.ptr(img), 50, 40, float(rho), float(theta), 5, float(lo), float(hi), vp.ptr(out), 8,
                                   vp.C.byref(n)) == -1, (rho, theta, lo, hi)
    assert L.vp_hough_lines_u8(ctx.handle, vp.ptr(img), 50, 40, 1e-6, STEP, 5, 0.0, np.pi, vp.ptr(out), 8, vp.C.byref(n)) == -4
    assert L.vp_hough_lines_u8(ctx.handle, vp.ptr(img), 50, 40, 1.0, 1e-7, 5, 0.0, np.pi, vp.ptr(out), 8, vp.C.byref(n)) == -4
    assert L.vp_hough_lines_u8(ctx.handle, vp.ptr(img), 0, 40, 1.0, STEP, 5, 0.0, np.pi, vp.ptr(out), 8, vp.C.byref(n)) == -1
    assert L.vp_hough_lines_u8(ctx.handle, vp.ptr(img), 50, 40, 1.0, STEP, 5, 0.0, np.pi, None, 8, vp.C.byref(n)) == -1
    assert L.vp_hough_lines_u8(ctx.handle, vp.ptr(img), 50, 40, 1.0, STEP, 5, 0.0, np.pi, vp.ptr(out), -1, vp.C.byref(n)) == -1
    with pytest.raises(vp.VpError):
        hough_lines(img, 1, 0, 5)
    # the context is still good afterwards
    _same(hough_lines(img, 1, STEP, 30), HR.hough_lines(img, 1, STEP, 30), "after errors")
