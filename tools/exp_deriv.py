"""Times the derivative filters (vp_deriv_dev, vp_spatial_gradient_dev, vp_convert_scale_abs_dev) on one 1080p device image.

    python tools/exp_deriv.py [--iters N] [--regions R]

One process, one GPU.  Every figure is the median over R regions of N back-to-back calls, each region bracketed by HIP events on the
context's stream.  One JSON line.  Per case: ms per call, the achieved bytes per second against the algorithmic bytes (1 byte read plus
sizeof(out) written per pixel-channel; spatialGradient writes two int16 planes, convertScaleAbs reads its source's element), and the
ratio of that rate to the rate vp_gaussian_blur_dev (3x3, the one-pass form, 1 read + 1 written) reaches on the same image in the same
run: the nearest existing stencil with the same read pattern.  The blur is timed before and after the cases; both visits are reported."""
import argparse
import json
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
from vision.devmat import DeviceMat  # noqa: E402

ctx = _vp.default_context()
lib = _vp.lib()
W, H = 1920, 1080
DEPTHS = {"8U": (_vp.DEPTH_8U, np.uint8), "16S": (_vp.DEPTH_16S, np.int16), "32F": (_vp.DEPTH_32F, np.float32), "64F": (_vp.DEPTH_64F, np.float64)}
B101 = _vp.BORDER_REFLECT_101


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
    blur_dst = {cn: DeviceMat(ctx, src[cn].shape) for cn in (1, 3)}
    ctx.set_option(_vp.OPT_BLUR_ONEPASS, 1)

    def blur(cn):
        def fn():
            _vp.check(lib.vp_gaussian_blur_dev(ctx.handle, src[cn].dev_ptr, W * cn, W, H, cn, 3, 3, 0.0, 0.0, blur_dst[cn].dev_ptr), ctx.handle)
        ms = median_ms(fn)
        return ms, 2.0 * W * H * cn / (ms * 1e-3)

    blur_first = {cn: blur(cn) for cn in (1, 3)}
    rows = []

    def row(name, cn, out, ms, nbytes):
        rows.append({"case": name, "cn": cn, "out": out, "ms": round(ms, 5), "bytes": int(nbytes), "bytes_per_s": round(nbytes / (ms * 1e-3), 0)})

    def deriv(name, cn, dname, op, dx, dy, k):
        depth, dtype = DEPTHS[dname]
        dst = DeviceMat(ctx, src[cn].shape, dtype)

        def fn():
            _vp.check(lib.vp_deriv_dev(ctx.handle, src[cn].dev_ptr, W * cn, W, H, cn, op, dx, dy, k, depth, B101, dst.dev_ptr), ctx.handle)
        row(name, cn, dname, median_ms(fn), W * H * cn * (1 + np.dtype(dtype).itemsize))

    for cn in (1, 3):
        for k in (3, 5, 7):
            for dname in ("8U", "16S", "32F"):
                deriv(f"Sobel(1,0,k={k})", cn, dname, _vp.DERIV_SOBEL, 1, 0, k)
    for cn in (1, 3):
        for k in (1, 3, 5, 7):
            deriv(f"Laplacian(k={k})", cn, "16S", _vp.DERIV_LAPLACIAN, 0, 0, k)
    deriv("Scharr(1,0)", 1, "16S", _vp.DERIV_SCHARR, 1, 0, 3)
    deriv("Sobel(1,0,k=3)", 1, "64F", _vp.DERIV_SOBEL, 1, 0, 3)
    gx, gy = DeviceMat(ctx, (H, W), np.int16), DeviceMat(ctx, (H, W), np.int16)

    def sg():
        _vp.check(lib.vp_spatial_gradient_dev(ctx.handle, src[1].dev_ptr, W, W, H, 3, B101, gx.dev_ptr, gy.dev_ptr), ctx.handle)
    row("spatialGradient", 1, "2x16S", median_ms(sg), W * H * 5)
    for cn in (1, 3):
        for dname in ("16S", "32F"):
            depth, dtype = DEPTHS[dname]
            plane = DeviceMat(ctx, src[cn].shape, dtype)
            _vp.check(lib.vp_deriv_dev(ctx.handle, src[cn].dev_ptr, W * cn, W, H, cn, _vp.DERIV_SOBEL, 1, 0, 3, depth, B101, plane.dev_ptr), ctx.handle)
            out = DeviceMat(ctx, src[cn].shape)

            def csa():
                _vp.check(lib.vp_convert_scale_abs_dev(ctx.handle, plane.dev_ptr, depth, W * H * cn, out.dev_ptr), ctx.handle)
            row(f"convertScaleAbs({dname})", cn, "8U", median_ms(csa), W * H * cn * (np.dtype(dtype).itemsize + 1))
    blur_second = {cn: blur(cn) for cn in (1, 3)}
    ctx.set_option(_vp.OPT_BLUR_ONEPASS, -1)
    for r in rows:
        ref = (blur_first[r["cn"]][1] + blur_second[r["cn"]][1]) / 2
        r["rate_vs_blur"] = round(r["bytes_per_s"] / ref, 3)
    print(json.dumps({"image": [H, W], "iters": args.iters, "regions": args.regions,
                      "blur3x3_onepass": {str(cn): {"ms": [round(blur_first[cn][0], 5), round(blur_second[cn][0], 5)],
                                                    "bytes_per_s": [round(blur_first[cn][1], 0), round(blur_second[cn][1], 0)]} for cn in (1, 3)},
                      "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
