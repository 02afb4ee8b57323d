"""Times the gathers (vp_remap_fixed_dev, vp_remap_f32_dev, vp_warp_perspective_dev) on one 1080p device image, grey and BGR.

    python tools/exp_remap.py [--iters N] [--regions R]

One process, one GPU.  Every figure is the median over R regions of N back-to-back calls, each region bracketed by HIP events on the
context's stream.  One JSON line.  Per case: ms per call and the achieved bytes per second against the algorithmic bytes (cn bytes
read and cn written per pixel, plus the map: 6 bytes of fixed form, 8 of float maps, none for the matrix forms).  The yardsticks run
in the same process: vp_warp_affine_dev of the same 30 degree rotation, and the 3x3 one-pass vp_gaussian_blur_dev, timed before and
after the cases; both visits are reported."""
import argparse
import json
import math
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--regions", type=int, default=9)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cuauv-vision-pipeline_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (shares the HIP runtime with libvp)

import frames as F  # noqa: E402
from vision import _vp  # noqa: E402
from vision import cv2_facade as cvf  # noqa: E402
from vision.devmat import DeviceMat  # noqa: E402
from vision.utils import transform  # noqa: E402

ctx = _vp.default_context()
lib = _vp.lib()
W, H = 1920, 1080


def median_ms(fn):
    for _ in range(3):
        fn()
    ctx.synchronize()
    t = []
    for _ in range(args.regions):
        ctx.timer_start()
        for _ in range(args.iters):
            fn()
        t.append(ctx.timer_stop() / args.iters)
    return statistics.median(t)


def main():
    bgr = F.s1_buoy(0, W, H)
    src = {1: DeviceMat.from_host(ctx, np.ascontiguousarray(bgr[:, :, 1])), 3: DeviceMat.from_host(ctx, bgr)}
    dst = {cn: DeviceMat(ctx, src[cn].shape) for cn in (1, 3)}
    bv = np.zeros(4, np.uint8)
    ctx.set_option(_vp.OPT_BLUR_ONEPASS, 1)

    def blur(cn):
        def fn():
            _vp.check(lib.vp_gaussian_blur_dev(ctx.handle, src[cn].dev_ptr, W * cn, W, H, cn, 3, 3, 0.0, 0.0, dst[cn].dev_ptr), ctx.handle)
        ms = median_ms(fn)
        return ms, 2.0 * W * H * cn / (ms * 1e-3)

    # the maps: identity, a barrel undistortion, the inverse of a 30 degree rotation about the centre
    yy, xx = np.mgrid[0:H, 0:W]
    K = np.array([[1400.0, 0.0, W / 2 - 0.5], [0.0, 1400.0, H / 2 - 0.5], [0.0, 0.0, 1.0]])
    a = math.radians(30.0)
    R23 = np.array([[math.cos(a), math.sin(a), 0.0], [-math.sin(a), math.cos(a), 0.0]])
    R23[:, 2] = np.array([W / 2, H / 2]) - R23[:, :2] @ np.array([W / 2, H / 2])          # source -> destination
    R33 = np.vstack([R23, [0.0, 0.0, 1.0]])
    Ri = np.linalg.inv(R33)
    maps = {"identity": (xx.astype(np.float32), yy.astype(np.float32)),
            "barrel": cvf.initUndistortRectifyMap(K, [-0.28, 0.09, 0.001, -0.0005, -0.01], None, K, (W, H), cvf.CV_32FC1),
            "rotate30": ((Ri[0, 0] * xx + Ri[0, 1] * yy + Ri[0, 2]).astype(np.float32), (Ri[1, 0] * xx + Ri[1, 1] * yy + Ri[1, 2]).astype(np.float32))}
    birdseye = cvf.getPerspectiveTransform([[W * 0.3, H * 0.35], [W * 0.7, H * 0.35], [W, H], [0, H]], [[0, 0], [W, 0], [W, H], [0, H]])

    blur_first = {cn: blur(cn) for cn in (1, 3)}
    rows = []

    def row(name, cn, ms, nbytes):
        rows.append({"case": name, "cn": cn, "ms": round(ms, 5), "bytes": int(nbytes), "bytes_per_s": round(nbytes / (ms * 1e-3), 0)})

    for cn in (1, 3):
        for name, (mx, my) in maps.items():
            table = transform.RemapTable(mx, my)

            def fixed():
                _vp.check(lib.vp_remap_fixed_dev(ctx.handle, src[cn].dev_ptr, W * cn, W, H, cn, table.xy.dev_ptr, table.frac.dev_ptr, W, H, _vp.INTER_LINEAR,
                                                 _vp.BORDER_CONSTANT, _vp.ptr(bv), dst[cn].dev_ptr), ctx.handle)
            row(f"RemapTable.apply({name})", cn, median_ms(fixed), W * H * (2 * cn + 6))
            dx, dy = DeviceMat.from_host(ctx, mx), DeviceMat.from_host(ctx, my)

            def f32():
                _vp.check(lib.vp_remap_f32_dev(ctx.handle, src[cn].dev_ptr, W * cn, W, H, cn, dx.dev_ptr, dy.dev_ptr, W, H, _vp.INTER_LINEAR, _vp.BORDER_CONSTANT,
                                               _vp.ptr(bv), dst[cn].dev_ptr), ctx.handle)
            row(f"remap(float maps, {name})", cn, median_ms(f32), W * H * (2 * cn + 8))
        for name, M in (("rotate30", R33), ("birdseye", birdseye)):
            m = np.ascontiguousarray(M, np.float64)

            def wp():
                _vp.check(lib.vp_warp_perspective_dev(ctx.handle, src[cn].dev_ptr, W * cn, W, H, cn, _vp.ptr(m), _vp.INTER_LINEAR, _vp.BORDER_CONSTANT, _vp.ptr(bv),
                                                      dst[cn].dev_ptr, W, H), ctx.handle)
            row(f"warpPerspective({name})", cn, median_ms(wp), W * H * 2 * cn)
        m23 = np.ascontiguousarray(R23, np.float64)

        def wa():
            _vp.check(lib.vp_warp_affine_dev(ctx.handle, src[cn].dev_ptr, W * cn, W, H, cn, _vp.ptr(m23), 0, _vp.BORDER_CONSTANT, _vp.ptr(bv), dst[cn].dev_ptr, W, H),
                      ctx.handle)
        row("warpAffine(rotate30)", cn, median_ms(wa), W * H * 2 * cn)
    blur_second = {cn: blur(cn) for cn in (1, 3)}
    ctx.set_option(_vp.OPT_BLUR_ONEPASS, -1)
    print(json.dumps({"image": [H, W], "iters": args.iters, "regions": args.regions,
                      "blur3x3_onepass": {str(cn): {"ms": [round(blur_first[cn][0], 5), round(blur_second[cn][0], 5)],
                                                    "bytes_per_s": [round(blur_first[cn][1], 0), round(blur_second[cn][1], 0)]} for cn in (1, 3)},
                      "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
