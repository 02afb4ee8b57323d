"""Times the box filter, the pyramid steps and the integral image (vp_box_filter_dev, vp_pyr_down_dev, vp_pyr_up_dev, vp_integral_dev)
on one 1080p device image, grey and BGR.

    python tools/exp_box_pyr.py [--iters N] [--regions R]

One process, one GPU.  Every figure is the median over R regions of N back-to-back calls, each region bracketed by HIP events on the
context's stream.  One JSON line.  Cases: blur at windows 3, 5, 15, 51 and 151 (with the path the plan chose), pyrDown, pyrUp of the
half-size image, integral.  Yardsticks, timed in the same run: vp_gaussian_blur_dev (3x3, the one-pass form) on the same image,
before and after the cases, and - grey only, it takes one channel - vp_adaptive_threshold_mean_dev at the same block sizes, the one
box sum the library had before (it does a threshold on top)."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--regions", type=int, default=7)
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
B101 = _vp.BORDER_REFLECT_101
WINDOWS = (3, 5, 15, 51, 151)


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
    ctx.set_option(_vp.OPT_BLUR_ONEPASS, 1)

    def gauss(cn):
        def fn():
            _vp.check(lib.vp_gaussian_blur_dev(ctx.handle, src[cn].dev_ptr, W * cn, W, H, cn, 3, 3, 0.0, 0.0, dst[cn].dev_ptr), ctx.handle)
        return median_ms(fn)

    gauss_first = {cn: gauss(cn) for cn in (1, 3)}
    rows = []
    for cn in (1, 3):
        for k in WINDOWS:
            def fn():
                _vp.check(lib.vp_box_filter_dev(ctx.handle, src[cn].dev_ptr, W * cn, W, H, cn, k, k, 1, -1, B101, dst[cn].dev_ptr), ctx.handle)
            r = {"case": f"blur({k})", "cn": cn, "ms": round(median_ms(fn), 5)}
            if cn == 1:
                def ad():
                    _vp.check(lib.vp_adaptive_threshold_mean_dev(ctx.handle, src[1].dev_ptr, W, W, H, 255.0, 0, k, 2.0, dst[1].dev_ptr), ctx.handle)
                r["adaptive_mean_ms"] = round(median_ms(ad), 5)
            rows.append(r)
        half = DeviceMat(ctx, ((H + 1) // 2, (W + 1) // 2) + src[cn].shape[2:])

        def down():
            _vp.check(lib.vp_pyr_down_dev(ctx.handle, src[cn].dev_ptr, W * cn, W, H, cn, B101, half.dev_ptr), ctx.handle)
        rows.append({"case": "pyrDown", "cn": cn, "ms": round(median_ms(down), 5)})
        hh, hw = half.shape[:2]
        full = DeviceMat(ctx, (2 * hh, 2 * hw) + src[cn].shape[2:])

        def up():
            _vp.check(lib.vp_pyr_up_dev(ctx.handle, half.dev_ptr, hw * cn, hw, hh, cn, full.dev_ptr), ctx.handle)
        rows.append({"case": "pyrUp(half)", "cn": cn, "ms": round(median_ms(up), 5)})
        sums = DeviceMat(ctx, (H + 1, W + 1) + src[cn].shape[2:], np.int32)

        def integ():
            _vp.check(lib.vp_integral_dev(ctx.handle, src[cn].dev_ptr, W * cn, W, H, cn, sums.dev_ptr), ctx.handle)
        rows.append({"case": "integral", "cn": cn, "ms": round(median_ms(integ), 5)})
    gauss_second = {cn: gauss(cn) for cn in (1, 3)}
    ctx.set_option(_vp.OPT_BLUR_ONEPASS, -1)
    print(json.dumps({"image": [H, W], "iters": args.iters, "regions": args.regions,
                      "gaussian3x3_onepass_ms": {str(cn): [round(gauss_first[cn], 5), round(gauss_second[cn], 5)] for cn in (1, 3)}, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
