"""Times the colour k-means (vp_kmeans_dev, vp_label_select_dev) on 1080p device images.

    python tools/exp_kmeans.py [--iters N] [--regions R]

One process, one GPU.  Every figure is the median over R regions of N back-to-back calls, each region bracketed by HIP events on the
context's stream.  One JSON line.  Images: the S1 frame, left / right halves of two colours, uniform noise; grey and BGR; k = 2, 4, 8
and 16, the initial centres k seeded pixels.  vp_kmeans_dev ends in one synchronise and a copy of the table, so every k-means figure
is a whole call and the parts are differences of whole calls, named for what they are:
  pass1_ms          max_iter = 1, no labels: the set-up launch, one assign-and-reduce pass, the update launch that ends the run, the
                    table back
  round_ms          (max_iter = 2) - (max_iter = 1) at eps = 0: one more assign pass and one update that moves the centres
  labels_ms         (max_iter = 1 with labels) - (max_iter = 1 without): the label write
  whole10_ms        iterations = 10, eps = 1.0, with labels: early convergence where the image allows it (`passes` says)
  whole10_end_ms    iterations = 10, eps = 0 (runs to the end unless no centre moves at all)
  idle_launch_us    ((max_iter = 100) - (max_iter = 10)) / 180 on the converged halves image: one launch that reads the state word
                    and returns
  floor_ms          pass1 on a 16 x 16 image of the same k and channels: what a call costs when the image costs nothing
  masks4_ms         mask_from_labels for 4 clusters (4 launches of vp_label_select_dev, bit planes included)
Yardsticks, timed in the same run before and after the cases: vp_hist_u8_dev, countNonZero and the 3x3 one-pass GaussianBlur of the
same image."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--regions", type=int, default=5)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cuauv-vision-pipeline_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (shares the HIP runtime with libvp)

import frames as F  # noqa: E402
from vision import _vp  # noqa: E402
from vision import cv2_facade as cv  # noqa: E402
from vision.devmat import DeviceMat  # noqa: E402
from vision.utils import color  # noqa: E402

ctx = _vp.default_context()
lib = _vp.lib()
W, H = 1920, 1080


def median_ms(fn):
    for _ in range(2):
        fn()
    ctx.synchronize()
    t = []
    for _ in range(args.regions):
        ctx.timer_start()
        for _ in range(args.iters):
            fn()
        t.append(ctx.timer_stop() / args.iters)
    return round(statistics.median(t), 5)


_SEEDS = {}


def run(img, k, max_iter, eps, labels):
    key = (img.shape[0] * img.shape[1], k)
    if key not in _SEEDS:               # (drawn outside the timed regions)
        _SEEDS[key] = color.kmeans_seed_indices(key[0], k, 1)
    return color.kmeans_run(img, k, max_iter, eps, seed_index=_SEEDS[key], labels=labels)


def main():
    rng = np.random.default_rng(7)
    s1 = F.s1_buoy(0, W, H)
    halves = np.zeros((H, W, 3), np.uint8)
    halves[:, :W // 2], halves[:, W // 2:] = (40, 90, 200), (180, 60, 20)
    noise = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    images = {}
    for name, bgr in (("S1 frame", s1), ("halves", halves), ("noise", noise)):
        images[name + ", BGR"] = DeviceMat.from_host(ctx, bgr)
        images[name + ", grey"] = DeviceMat.from_host(ctx, np.ascontiguousarray(bgr[:, :, 1]))
    grey = images["noise, grey"]
    blurred = DeviceMat(ctx, (H, W), np.uint8)
    hist = np.zeros(256, np.uint32)

    def yard():
        def gauss():
            _vp.check(lib.vp_gaussian_blur_dev(ctx.handle, grey.dev_ptr, W, W, H, 1, 3, 3, 0.0, 0.0, blurred.dev_ptr), ctx.handle)

        def histogram():
            _vp.check(lib.vp_hist_u8_dev(ctx.handle, grey.dev_ptr, W * H, hist.ctypes.data), ctx.handle)
        return {"hist_u8_ms": median_ms(histogram), "count_nonzero_ms": median_ms(lambda: cv.countNonZero(grey)), "gaussian_3x3_ms": median_ms(gauss)}

    first = yard()
    rows = []
    for name, img in images.items():
        tiny = DeviceMat.from_host(ctx, np.ascontiguousarray(img.host(writable=False)[:16, :16]))
        for k in (2, 4, 8, 16):
            one = median_ms(lambda: run(img, k, 1, 0.0, False))
            row = {"image": name, "k": k, "pass1_ms": one, "round_ms": round(median_ms(lambda: run(img, k, 2, 0.0, False)) - one, 5),
                   "labels_ms": round(median_ms(lambda: run(img, k, 1, 0.0, True)) - one, 5),
                   "whole10_ms": median_ms(lambda: run(img, k, 10, 1.0, True)), "passes": run(img, k, 10, 1.0, False)[4],
                   "whole10_end_ms": median_ms(lambda: run(img, k, 10, 0.0, True)), "passes_end": run(img, k, 10, 0.0, False)[4],
                   "floor_ms": median_ms(lambda: run(tiny, k, 1, 0.0, False))}
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    conv = images["halves, BGR"]
    assert run(conv, 2, 100, 1.0, False)[4] < 10
    idle = (median_ms(lambda: run(conv, 2, 100, 1.0, False)) - median_ms(lambda: run(conv, 2, 10, 1.0, False))) / 180.0
    _c, labels, centres, _n, _p = run(images["S1 frame, BGR"], 4, 10, 1.0, True)
    masks = median_ms(lambda: color.mask_from_labels(labels, centres))
    second = yard()
    print(json.dumps({"image": [H, W], "iters": args.iters, "regions": args.regions, "yardsticks_first": first, "yardsticks_second": second,
                      "idle_launch_us": round(idle * 1000.0, 3), "masks4_ms": masks, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
