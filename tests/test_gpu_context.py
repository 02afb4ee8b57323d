"""GPU suite for the context unit (csrc/vp_api.hip, vp_options.h): vp_set_option accepts exactly the documented range of every option,
and a context that has made every unit set up its lazily allocated state - labelling, HoughCircles, the Gaussian adaptive threshold,
contours, posts, the profile - is created, used and destroyed eight times over with the same results each time.  The failure exits
of vp_create are not provoked here."""
import ctypes as C
from contextlib import contextmanager

import numpy as np
import pytest

from test_options_host import INT_MAX, ROWS

pytestmark = pytest.mark.gpu


@contextmanager
def _as_default(vp, ctx):
    """The mirror's operators run on the calling thread's default context: make `ctx` that one for a while."""
    saved = getattr(vp._tls, "ctxs", None)
    vp._tls.ctxs = {0: ctx}
    try:
        yield ctx
    finally:
        vp._tls.ctxs = saved


def test_every_option_accepts_exactly_its_range(vp):
    L = vp.lib()
    ctx = vp.Context(0)
    try:
        for oid, name, lo, hi, dflt, _env in ROWS:
            assert getattr(vp, "OPT_" + name) == oid
            assert L.vp_set_option(ctx.handle, oid, lo) == 0, (name, lo)
            assert L.vp_set_option(ctx.handle, oid, hi) == 0, (name, hi)
            assert L.vp_set_option(ctx.handle, oid, lo - 1) == -1, (name, lo - 1)
            if hi < INT_MAX:                                  # CCL_MERGE_CAP has no value above its range: refused only at -2
                assert L.vp_set_option(ctx.handle, oid, hi + 1) == -1, (name, hi + 1)
            assert L.vp_last_error(ctx.handle) == b"vp_set_option"
            assert L.vp_set_option(ctx.handle, oid, dflt) == 0, (name, dflt)
        for oid in (0, 12, 77):
            assert L.vp_set_option(ctx.handle, oid, 1) == -1, oid
            assert L.vp_last_error(ctx.handle) == b"vp_set_option" and L.vp_last_error(None) == b"vp_set_option"
    finally:
        ctx.close()


def _ring(side=64, r=20, t=2):
    y, x = np.mgrid[:side, :side]
    d = np.hypot(x - side / 2, y - side / 2)
    return np.where(np.abs(d - r) <= t, 255, 0).astype(np.uint8)


def _post_roundtrip(vp, ctx, payload):
    """one vp_post_d2h of the payload (device -> a vp_host_alloc buffer), waited for and freed"""
    L = vp.lib()
    n = payload.nbytes
    dev, host, done = C.c_void_p(), C.c_void_p(), C.c_void_p()
    vp.check(L.vp_dev_alloc(ctx.handle, n, C.byref(dev)), ctx.handle)
    vp.check(L.vp_host_alloc(ctx.handle, n, C.byref(host)), ctx.handle)
    try:
        vp.check(L.vp_memcpy_h2d(ctx.handle, dev, vp.ptr(payload), n), ctx.handle)
        vp.check(L.vp_post_d2h(ctx.handle, 0, host, dev, n, C.byref(done)), ctx.handle)
        vp.check(L.vp_post_wait(ctx.handle, done), ctx.handle)
        assert L.vp_post_done(ctx.handle, done) == 1
        vp.check(L.vp_post_free(ctx.handle, done), ctx.handle)
        return C.string_at(host.value, n)
    finally:
        vp.check(L.vp_host_free(ctx.handle, host), ctx.handle)
        vp.check(L.vp_dev_free(ctx.handle, dev), ctx.handle)


def _use_every_stateful_unit(vp):
    """a fresh context, one small call into each unit that keeps state on it, close(); -> the outputs as bytes"""
    from vision.utils import color, feature
    rng = np.random.default_rng(11)
    mask = (rng.random((48, 64)) < 0.5).astype(np.uint8) * 255
    grey = rng.integers(0, 256, (17, 33), dtype=np.uint8)
    small = np.zeros((16, 16), np.uint8)
    small[3:9, 2:12] = 255
    small[5:7, 5:8] = 0
    small[12:15, 9:15] = 255
    payload = rng.integers(0, 256, 4096, dtype=np.uint8)
    out = []
    ctx = vp.Context(0)
    try:
        with _as_default(vp, ctx):
            ctx.set_option(vp.OPT_CCL_CROWDED, 1)
            ctx.profile_begin(8)
            n, labels, stats, cent = feature.connected_components(mask)
            prof = ctx.profile_end()
            assert n > 2 and sum(cnt for _ms, cnt in prof.values()) >= 1, (n, prof)
            out += [np.int64(n).tobytes(), labels.tobytes(), stats.tobytes(), cent.tobytes()]
            ctx.set_option(vp.OPT_HOUGH_CIRCLES_LDS, 0)
            circles = feature.hough_circles(_ring(), 1, 16, 100, 10, 10, 30)
            assert circles is not None and circles.shape[1] >= 1
            out.append(circles.tobytes())
            thr = color.adaptive_threshold_gaussian(grey, 5)
            assert thr.shape == grey.shape and 0 < np.count_nonzero(thr) < thr.size
            out.append(np.ascontiguousarray(thr).tobytes())
            contours = feature.find_contours(small, vp.RETR_LIST, vp.CHAIN_APPROX_SIMPLE)
            assert len(contours) == 3
            out += [c.tobytes() for c in contours]
            back = _post_roundtrip(vp, ctx, payload)
            assert back == payload.tobytes()
            out.append(back)
    finally:
        ctx.close()
    assert ctx.handle is None
    return out


def test_eight_lifetimes_give_the_same_results(vp):
    first = _use_every_stateful_unit(vp)
    for i in range(1, 8):
        again = _use_every_stateful_unit(vp)
        assert len(again) == len(first) and all(a == b for a, b in zip(again, first)), f"lifetime {i + 1} differs from the first"
    assert vp.lib().vp_destroy(None) == -1
    vp.default_context().synchronize()                       # the thread's own context is untouched by all of it
