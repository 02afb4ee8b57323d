"""Times the corner operators (vp_corner_response_dev, vp_good_features_dev) on one 1080p device image.

    python tools/exp_corners.py [--iters N] [--regions R]

One process, one GPU.  Every figure is the median over R regions of N back-to-back calls, each region bracketed by HIP events on the
context's stream.  One JSON line.  Images: grey noise, the green channel of the S1 frame, a checkerboard of 16-pixel cells.  Cases: the
response map at blockSize 3, 7 and 15, min eigenvalue and Harris, written to a device image made once; the whole
good_features_to_track (response, maximum, candidates, their order, the count and the ordered words copied back, the greedy pass on the
host) at max_corners 100 and 0, min_distance 10, with the candidate count of each image.  Yardsticks, timed in the same run before and
after the cases on the noise image: Sobel(1, 0) to float32 (one byte read, four written per pixel, like the response map) and the
3x3 one-pass GaussianBlur."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--regions", type=int, default=7)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cuauv-vision-pipeline_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (shares the HIP runtime with libvp)

import frames as F  # noqa: E402
from vision import _vp  # noqa: E402
from vision.devmat import DeviceMat  # noqa: E402
from vision.utils import feature  # noqa: E402

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
    return round(statistics.median(t), 5)


def main():
    rng = np.random.default_rng(7)
    yy, xx = np.indices((H, W))
    images = [("grey noise", rng.integers(0, 256, (H, W), dtype=np.uint8)),
              ("S1 frame", np.ascontiguousarray(F.s1_buoy(0, W, H)[:, :, 1])),
              ("checkerboard", (((yy // 16 + xx // 16) % 2) * 255).astype(np.uint8))]
    dev = [(name, DeviceMat.from_host(ctx, img)) for name, img in images]
    resp = DeviceMat(ctx, (H, W), np.float32)
    blurred = DeviceMat(ctx, (H, W), np.uint8)

    def yard():
        src = dev[0][1]

        def sobel():
            _vp.check(lib.vp_deriv_dev(ctx.handle, src.dev_ptr, W, W, H, 1, _vp.DERIV_SOBEL, 1, 0, 3, _vp.DEPTH_32F, _vp.BORDER_REFLECT_101, resp.dev_ptr), ctx.handle)

        def gauss():
            _vp.check(lib.vp_gaussian_blur_dev(ctx.handle, src.dev_ptr, W, W, H, 1, 3, 3, 0.0, 0.0, blurred.dev_ptr), ctx.handle)
        return {"sobel_f32_ms": median_ms(sobel), "gaussian_3x3_ms": median_ms(gauss)}

    first = yard()
    rows = []
    for name, src in dev:
        for block in (3, 7, 15):
            for harris in (0, 1):
                def fn():
                    _vp.check(lib.vp_corner_response_dev(ctx.handle, src.dev_ptr, W, W, H, block, 3, harris, 0.04, _vp.BORDER_REFLECT_101, resp.dev_ptr), ctx.handle)
                rows.append({"case": "response", "image": name, "block": block, "harris": harris, "ms": median_ms(fn)})
        for max_corners in (100, 0):
            found = feature.good_features_to_track(src, max_corners, 0.01, 10)
            rows.append({"case": "good_features_to_track", "image": name, "max_corners": max_corners, "corners": 0 if found is None else len(found),
                         "ms": median_ms(lambda: feature.good_features_to_track(src, max_corners, 0.01, 10))})
    second = yard()
    print(json.dumps({"image": [H, W], "iters": args.iters, "regions": args.regions, "yardsticks_first": first, "yardsticks_second": second, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
