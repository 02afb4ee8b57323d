"""GPU suite: one context's workspace grows across operators of very different needs, and no call sees another's layout.  Every call
declares its buffers on a frame and commits it once (csrc/vp_ws_frame.h, vp_ws_commit); a pointer wired to the wrong region, or a
region that moved when the workspace was reallocated, shows as a result that differs from the same call on a context of its own."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _threshold(vp, ctx, img):
    out = np.empty_like(img)
    vp.check(vp.lib().vp_threshold_u8(ctx.handle, vp.ptr(img), img.size, 100.0, 255.0, 0, vp.ptr(out)), ctx.handle)
    return [out]


def _blur(vp, ctx, img):
    h, w, cn = img.shape
    out = np.empty_like(img)
    vp.check(vp.lib().vp_gaussian_blur_u8(ctx.handle, vp.ptr(img), w, h, cn, 5, 5, 0.0, 0.0, vp.ptr(out)), ctx.handle)
    return [out]


def _circles(vp, ctx, img):
    out = np.full((64, 3), -1.0, np.float32)
    n = vp.C.c_int(-1)
    vp.check(vp.lib().vp_hough_circles_u8(ctx.handle, vp.ptr(img), img.shape[1], img.shape[0], 1.0, 8.0, 100.0, 15.0, 0, 0, vp.ptr(out), 64, vp.C.byref(n)),
             ctx.handle)
    return [np.array([n.value]), out]


def _chain_contours(vp, ctx, frames):
    n, h, w, _ = frames.shape
    ml = 64
    desc = vp.make_chain_desc(w, h, vp.BGR2LAB, (0, 150, 0), (255, 255, 255), [(vp.MORPH_OPEN, 3, 3), (vp.MORPH_CLOSE, 3, 3)], 1, vp.CCL_BLOCK2X2, ml)
    bufs = vp.ChainBuffers()
    out = dict(threshed=np.zeros((n, h, w), np.uint8), cleaned=np.zeros((n, h, w), np.uint8), labels=np.zeros((n, h, w), np.int32),
               stats=np.zeros((n, ml, 5), np.int32), centroids=np.zeros((n, ml, 2), np.float64), nlabels=np.zeros((n,), np.int32))
    bufs.bgr = frames.ctypes.data
    for k, a in out.items():
        setattr(bufs, k, a.ctypes.data)
    cdesc = vp.make_contour_desc(source="cleaned", mode=1, method=2, max_contours=32, max_points=2048)
    arrs, cb = vp.contour_arrays(lambda shape, dt: np.zeros(shape, dt), n, cdesc)
    ctx.set_option(vp.OPT_CHAIN_STREAMS, 4)
    ctx.chain_run_contours_host(desc, bufs, cdesc, cb, n)
    res = [out[k] for k in ("threshed", "cleaned", "labels", "nlabels")]
    for f in range(n):                                     # rows past a frame's count hold whatever the workspace held: compare what is defined
        nl = int(out["nlabels"][f])
        res += [out["stats"][f, :nl].copy(), out["centroids"][f, :nl].copy()]
    res.append(arrs["info"].copy())
    for f in range(n):
        nc, npts = int(arrs["info"][f, 0]), int(arrs["info"][f, 1])
        assert 0 < nc <= cdesc.max_contours and npts <= cdesc.max_points, "the frames are meant to have contours within the capacity"
        res += [arrs[k][f, :nc].copy() for k in ("counts", "offsets", "is_hole", "features")] + [arrs["points"][f, :npts].copy()]
    return res


def test_growth_across_operators_on_one_context_changes_no_result(vp):
    rng = np.random.default_rng(11)
    small = rng.integers(0, 256, (48, 64), dtype=np.uint8)                      # far below 1 MiB
    big = rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)                   # forces a reallocation
    yy, xx = np.mgrid[0:64, 0:96]
    discs = np.full((64, 96), 30, np.uint8)
    for cx, cy, r in ((30, 30, 18), (68, 36, 14)):
        discs[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 220
    frames = np.zeros((5, 38, 70, 3), np.uint8)
    frames[...] = (90, 90, 90)
    for f in range(5):
        frames[f, 5 + f:20 + f, 8 + 2 * f:30 + 2 * f] = (40, 40, 230)           # a red block (Lab a above 150) that moves
        frames[f, 24:34, 44 + f:62 + f] = (30, 30, 200)
        frames[f, 27:30, 50 + f:54 + f] = (90, 90, 90)                          # with a hole in the second
    steps = [(_threshold, small), (_blur, big), (_circles, discs), (_chain_contours, frames), (_threshold, small)]
    shared = vp.Context()
    try:
        for i, (call, arg) in enumerate(steps):
            got = call(vp, shared, arg)
            alone = vp.Context()
            try:
                exp = call(vp, alone, arg)
            finally:
                alone.close()
            assert len(got) == len(exp)
            for j, (a, b) in enumerate(zip(got, exp)):
                assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"step {i} ({call.__name__}), result {j} differs from the fresh context's"
            if call is _circles:
                assert got[0][0] == 2, "both drawn circles are meant to be found"
    finally:
        shared.close()
