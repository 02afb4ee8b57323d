"""Element-wise operators on resident 1080p images against the host path they replace: `a & b` of two masks, split -> add(bias) ->
merge of a BGR frame, countNonZero.  Device column: HIP events around a warmed-up loop of `calls` launches (device ms per call) and the
wall clock around the same loop, synchronised at its end.  Host column: what the operators did before (and still do with VP_LAZY=0 or
numpy input) - every device operand downloaded afresh, as a new frame's would be, then the numpy statements; the upload the next
operator would need is not counted.  Also each kernel's share of the HBM peak from its algorithmic bytes, beside vp_add_weighted_u8_dev
for the same byte count.
usage: python tools/exp_elementwise.py [calls]        (json on the last line)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "cuauv-vision-pipeline_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import frames as F
from vision import _vp, cv2_facade as cv2, devmat
from vision.devmat import DeviceMat
from vision.utils import color

HBM_PEAK = 8.0e12          # bytes / s (MI355X data sheet)


def _fresh(*mats):
    """Forget the cached host copies: the next read downloads, as it would for the masks of a new frame."""
    for m in mats:
        m._host = None


def _device(ctx, fn, calls):
    for _ in range(10):
        fn()
    ctx.synchronize()
    t0 = time.perf_counter()
    ctx.timer_start()
    for _ in range(calls):
        fn()
    ms = ctx.timer_stop()
    wall = time.perf_counter() - t0
    return ms / calls, 1e3 * wall / calls


def _host(fn, calls):
    for _ in range(3):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def measure(calls=200):
    ctx = _vp.default_context()
    frame = F.s1_buoy(0)
    h, w = frame.shape[:2]
    lab_a = color.bgr_to_lab(frame)[1][1]
    a, b = color.range_threshold(lab_a, 150, 255), color.range_threshold(color.bgr_to_gray(frame)[1][0], 60, 255)
    bgr = DeviceMat.from_host(ctx, frame)
    out = {"size": [w, h], "calls": calls}

    def row(name, dev_fn, host_fn, nbytes):
        dev_ms, wall_ms = _device(ctx, dev_fn, calls)
        host_ms = _host(host_fn, max(5, calls // 10))
        out[name] = {"device_ms": round(dev_ms, 5), "device_wall_ms": round(wall_ms, 5), "host_ms": round(host_ms, 4), "algorithmic_bytes": nbytes,
                     "hbm_share": round(nbytes / (dev_ms * 1e-3) / HBM_PEAK, 4)}

    def host_and():
        _fresh(a, b)
        devmat.set_lazy(False)
        try:
            return a & b
        finally:
            devmat.set_lazy(True)
    row("mask_and", lambda: (a & b).dev_ptr, host_and, 3 * w * h + w * h // 8)

    def dev_bias():
        p = list(cv2.split(bgr))
        p[2] = cv2.add(17, p[2])
        return cv2.merge(p).dev_ptr

    def host_bias():
        _fresh(bgr)
        p = list(cv2.split(bgr.host(writable=False)))
        p[2] = cv2.add(17, p[2])
        return cv2.merge(p)
    row("split_add_merge", dev_bias, host_bias, (6 + 2 + 6) * w * h)

    nz = np.count_nonzero(np.asarray(a.host_copy()))

    def dev_count():
        assert cv2.countNonZero(a) == nz

    def host_count():
        _fresh(a)
        assert np.count_nonzero(a.host(writable=False)) == nz
    row("count_non_zero", dev_count, host_count, w * h)

    # the single kernels, launch after launch into one destination, and addWeighted for the same bytes
    lib, n = _vp.lib(), 3 * w * h
    x, y, z = DeviceMat.from_host(ctx, frame), DeviceMat.from_host(ctx, frame[::-1].copy()), DeviceMat(ctx, frame.shape)
    planes = cv2.split(bgr)
    lut = np.arange(256, dtype=np.uint8)[::-1].copy()
    px, py, pz, pp = x.dev_ptr, y.dev_ptr, z.dev_ptr, [p.dev_ptr for p in planes]
    kernels = {
        "bitwise_and_3ch": (lambda: lib.vp_bitwise_u8_dev(ctx.handle, _vp.BITWISE_AND, px, py, 0, None, 1, n, pz, 0, None, None), 3 * n),
        "arith_add_3ch": (lambda: lib.vp_arith_u8_dev(ctx.handle, _vp.ARITH_ADD, px, py, n, pz), 3 * n),
        "add_weighted_3ch": (lambda: lib.vp_add_weighted_u8_dev(ctx.handle, px, 0.5, py, 0.5, 0.0, n, pz), 3 * n),
        "lut_3ch": (lambda: lib.vp_lut_u8_dev(ctx.handle, px, n, 1, lut.ctypes.data, pz), 2 * n),
        "split_3ch": (lambda: lib.vp_split_u8_dev(ctx.handle, px, w * h, 3, pp[0], pp[1], pp[2], None), 2 * n),
        "merge_3ch": (lambda: lib.vp_merge_u8_dev(ctx.handle, pp[0], pp[1], pp[2], None, w * h, 3, pz), 2 * n),
    }
    out["kernels"] = {}
    for name, (fn, nbytes) in kernels.items():
        dev_ms, _ = _device(ctx, fn, calls)
        out["kernels"][name] = {"device_ms": round(dev_ms, 5), "algorithmic_bytes": nbytes, "hbm_share": round(nbytes / (dev_ms * 1e-3) / HBM_PEAK, 4)}
    return out


if __name__ == "__main__":
    r = measure(int(sys.argv[1]) if len(sys.argv) > 1 else 200)
    for k, v in r.items():
        print(k, v)
    print(json.dumps(r))
