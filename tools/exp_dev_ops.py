"""Times the operators that take a device image, on 1080p frames that a device operator produced.

    python tools/exp_dev_ops.py [--part ops|blur|body|calls|all] [--iters N] [--regions R] [--root DIR]

One process, one GPU.  Every figure is the median over R regions of N back-to-back calls, each region bracketed by HIP events on the
context's stream (host time spent inside a call that waits for the device is part of the region, as it is for a module).  One JSON line
per part.

  ops   per operator (BGR for blur / resize / warp, grey for thresholds and labelling): ms per call with a DeviceMat argument.  Each call
        gets a fresh image from a device operator (a commit that fetches its input to the host then pays for that every time, as a
        module would); the producer's own time is measured alone and subtracted.
  blur  vp_gaussian_blur_dev with VP_OPT_BLUR_ONEPASS 1 against 0 in the same run, cn 1 and 3, k 3 .. 31 (builds with the option only).
  body  the red_buoy harness body behind a leading simple_gaussian_blur(image, 5, 0), posts off and on, frame given as a DeviceMat.
  calls calls per second of the device form of every operator of the Python operator layer on a 64 x 64
        image, where a call is bound by its launch and by the Python around it: host time of N back-to-back calls and one wait for
        the device.  Not part of `all`: it is run on two checkouts in turn (--root), several times each.

--root DIR imports the package (and tests/frames.py, tests/module_harness.py) of another checkout, built there, so that the same script
times the parent commit: `ops`, `body` and `calls` use only names the mirror has always had."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--part", default="all")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--regions", type=int, default=7)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path[:0] = [ROOT, os.path.join(ROOT, "cuauv-vision-pipeline_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (shares the HIP runtime with libvp)

import frames as F  # noqa: E402
from vision import _vp  # noqa: E402
from vision.devmat import DeviceMat  # noqa: E402
from vision.utils import color, feature, transform  # noqa: E402

ctx = _vp.default_context()
W, H = 1920, 1080


def median_ms(fn, iters=None, regions=None):
    """median over regions of (HIP-event time of `iters` back-to-back calls) / iters"""
    iters, regions = iters or args.iters, regions or args.regions
    for _ in range(3):
        fn()
    ctx.synchronize()
    t = []
    for _ in range(regions):
        ctx.timer_start()
        for _ in range(iters):
            fn()
        t.append(ctx.timer_stop() / iters)
    return round(statistics.median(t), 5)


def part_ops():
    frame = DeviceMat.from_host(ctx, F.s1_buoy(0, W, H))

    def fresh_bgr():                                  # a BGR image that a device operator has just produced
        return color.bgr_to_lab(frame)[0]

    def fresh_gray():
        return color.bgr_to_gray(frame)[0]

    def fresh_mask():
        return color.range_threshold(color.bgr_to_gray(frame)[0], 100, 255)
    out = {"part": "ops", "image": [H, W], "iters": args.iters, "regions": args.regions, "root": ROOT}
    prod = {"bgr": median_ms(lambda: fresh_bgr()), "gray": median_ms(lambda: fresh_gray()), "mask": median_ms(lambda: fresh_mask())}
    out["producer_ms"] = prod
    ops = [("simple_gaussian_blur_5", "bgr", fresh_bgr, lambda m: transform.simple_gaussian_blur(m, 5, 0)),
           ("simple_gaussian_blur_31", "bgr", fresh_bgr, lambda m: transform.simple_gaussian_blur(m, 31, 0)),
           ("resize_960x540", "bgr", fresh_bgr, lambda m: transform.resize(m, 960, 540)),
           ("resize_1280x720", "bgr", fresh_bgr, lambda m: transform.resize(m, 1280, 720)),
           ("rotate_10", "bgr", fresh_bgr, lambda m: transform.rotate(m, 10.0)),
           ("translate", "bgr", fresh_bgr, lambda m: transform.translate(m, 12, 7)),
           ("max_threshold", "gray", fresh_gray, lambda m: color.max_threshold(m, 120)),
           ("above_threshold", "gray", fresh_gray, lambda m: color.above_threshold(m, 120)),
           ("otsu_threshold", "gray", fresh_gray, lambda m: color.otsu_threshold(m)),
           ("adaptive_threshold_mean_15", "gray", fresh_gray, lambda m: color.adaptive_threshold_mean(m, 15, 2)),
           ("simple_canny", "gray", fresh_gray, lambda m: feature.simple_canny(m)),
           ("connected_components_stats", "mask", fresh_mask, lambda m: feature.connected_components(m, want_labels=False)),
           ("connected_components_labels", "mask", fresh_mask, lambda m: feature.connected_components(m))]
    res = {}
    for name, kind, make, op in ops:
        both = median_ms(lambda: op(make()))
        res[name] = {"with_producer_ms": both, "ms": round(both - prod[kind], 5)}
    out["ops"] = res
    print(json.dumps(out), flush=True)


def part_blur():
    lib = _vp.lib()
    out = {"part": "blur", "image": [H, W], "iters": 50, "regions": args.regions}
    bgr = F.s1_buoy(0, W, H)
    rows = []
    try:
        for cn in (1, 3):
            img = np.ascontiguousarray(bgr[:, :, 1]) if cn == 1 else bgr
            src = DeviceMat.from_host(ctx, img)
            dst = DeviceMat(ctx, img.shape)
            for k in (3, 5, 7, 11, 15, 21, 31):
                def fn():
                    _vp.check(lib.vp_gaussian_blur_dev(ctx.handle, src.dev_ptr, W * cn, W, H, cn, k, k, 0.0, 0.0, dst.dev_ptr), ctx.handle)
                t = {}
                for opt in (0, 1, 0, 1):                  # each form twice, interleaved: drift shows as a gap between the two visits
                    ctx.set_option(_vp.OPT_BLUR_ONEPASS, opt)
                    t.setdefault(opt, []).append(median_ms(fn, iters=50))
                rows.append({"cn": cn, "k": k, "two_pass_ms": t[0], "one_pass_ms": t[1]})
    finally:
        ctx.set_option(_vp.OPT_BLUR_ONEPASS, -1)
    out["rows"] = rows
    print(json.dumps(out), flush=True)


def part_body():
    import module_harness as MH
    normal = np.zeros((8, 8, 3), np.float32)
    base = [F.s1_buoy(i, W, H) for i in range(4)]
    out = {"part": "body", "image": [H, W], "root": ROOT}
    calls = 40
    for posts in (False, True):
        me = MH.PlainSelf((H, W), posts, tag="Exp%d" % int(posts))
        t = []
        for region in range(args.regions + 1):
            imgs = [DeviceMat.from_host(ctx, base[i % 4]) for i in range(calls)]
            ctx.synchronize()
            ctx.timer_start()
            for img in imgs:
                MH.buoy_body(me, transform.simple_gaussian_blur(img, 5, 0), normal)
                me.flush()
            t.append(ctx.timer_stop() / calls)
        me.close()
        out["posts_on_ms" if posts else "posts_off_ms"] = round(statistics.median(t[1:]), 5)      # the first region warms up
    print(json.dumps(out), flush=True)


def part_calls():
    from vision import cv2_facade as f
    rng = np.random.default_rng(64)
    grey = DeviceMat.from_host(ctx, rng.integers(0, 256, (64, 64), dtype=np.uint8))
    bgr = DeviceMat.from_host(ctx, rng.integers(0, 256, (64, 64, 3), dtype=np.uint8))
    mask = DeviceMat.from_host(ctx, np.where(rng.random((64, 64)) < 0.4, 255, 0).astype(np.uint8), binary=True)
    signed = transform.sobel(grey, 1, 0)
    mx, my = (DeviceMat.from_host(ctx, (rng.random((64, 64), dtype=np.float32) * 66 - 1).astype(np.float32)) for _ in range(2))
    M = np.array([[1.05, 0.08, -0.6], [-0.04, 0.97, 0.8], [0.0003, -0.0002, 1.0]])
    ops = [("simple_gaussian_blur", lambda: transform.simple_gaussian_blur(bgr, 5, 0)), ("GaussianBlur", lambda: f.GaussianBlur(bgr, (5, 5), 0)),
           ("resize", lambda: transform.resize(bgr, 48, 40)), ("rotate", lambda: transform.rotate(bgr, 10.0)), ("translate", lambda: transform.translate(bgr, 3, 2)),
           ("median_blur", lambda: transform.median_blur(bgr, 3)), ("median_blur_mask", lambda: transform.median_blur(mask, 3)),
           ("sobel", lambda: transform.sobel(bgr, 1, 0)), ("Sobel", lambda: f.Sobel(bgr, f.CV_16S, 1, 0)), ("scharr", lambda: transform.scharr(bgr, 1, 0)),
           ("laplacian", lambda: transform.laplacian(bgr, 3)), ("spatial_gradient", lambda: transform.spatial_gradient(grey)),
           ("convert_scale_abs", lambda: transform.convert_scale_abs(signed)), ("box_filter", lambda: transform.box_filter(bgr, 3)),
           ("blur", lambda: f.blur(bgr, (3, 3))), ("pyr_down", lambda: transform.pyr_down(bgr)), ("pyr_up", lambda: transform.pyr_up(bgr)),
           ("integral", lambda: transform.integral(bgr)), ("equalize_hist", lambda: color.equalize_hist(grey)), ("clahe", lambda: color.clahe(grey, 2.0, (4, 4))),
           ("remap", lambda: transform.remap(bgr, mx, my)), ("warp_perspective", lambda: transform.warp_perspective(bgr, M, 64, 64))]
    n = args.iters * 25
    res = {}
    for name, op in ops:
        for _ in range(20):
            op()
        ctx.synchronize()
        t = []
        for _ in range(args.regions):
            t0 = time.perf_counter()
            for _ in range(n):
                op()
            ctx.synchronize()
            t.append(n / (time.perf_counter() - t0))
        res[name] = round(statistics.median(t))
    print(json.dumps({"part": "calls", "image": [64, 64], "calls": n, "regions": args.regions, "root": ROOT, "calls_per_s": res}), flush=True)


if __name__ == "__main__":
    if args.part == "calls":
        part_calls()
    for name, fn in (("ops", part_ops), ("blur", part_blur), ("body", part_body)):
        if args.part in (name, "all"):
            fn()
