"""Times robust motion estimation from point pairs (vision.utils.feature.estimate_motion; libvp vp_estimate_model_f32, vp_model.hip).

    python tools/exp_model.py [--iters N] [--regions R]

One process, one GPU.  Every device figure is the median over R regions of N back-to-back calls, each region bracketed by HIP events on
the context's stream; every call is whole and synchronised (it stages its points, enqueues all rounds, brings the mask back and refits
on the host).  One JSON line.  The three models at 100, 1,000, 10,000 and 100,000 pairs with 0, 30 and 60 % outliers (an exact model on
[0, 2048)^2, the outliers uniform noise; defaults: threshold 3, max_iters 2000, confidence 0.99); next to each the host form of the same
statement, vp_estimate_model_host, on the same input in the same run (host clock, best of `--host-runs`).  Then the cost of one further
round (a search that cannot stop, max_iters 512 against 256) and of an idle round (a search that stops in round 1, max_iters 2000
against 256, over the seven rounds behind it).  Yardstick: track_points of 1,000 points between two 1080p frames over ready pyramids."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--regions", type=int, default=5)
ap.add_argument("--host-runs", type=int, default=2)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cuauv-vision-pipeline_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (shares the HIP runtime with libvp)

from vision import _vp  # noqa: E402
from vision.devmat import DeviceMat  # noqa: E402
from vision.utils import feature  # noqa: E402

ctx = _vp.default_context()
MODELS = ("similarity", "affine", "homography")


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
    return round(statistics.median(t), 5), round(max(t) - min(t), 5)


def pairs(n, model, outliers, seed=0):
    r = np.random.default_rng(seed + 17 * n)
    ang, sc = 0.12, 1.07
    H = np.eye(3)
    H[:2, :2] = sc * np.array([[math.cos(ang), -math.sin(ang)], [math.sin(ang), math.cos(ang)]])
    H[:2, 2] = (31.5, -18.25)
    if model != "similarity":
        H[:2, :2] += [[0.03, -0.02], [0.01, 0.04]]
    if model == "homography":
        H[2, :2] = (2e-5, -3e-5)
    src = r.uniform(0, 2048, (n, 2)).astype(np.float32)
    s = np.concatenate([src.astype(np.float64), np.ones((n, 1))], 1) @ H.T
    dst = (s[:, :2] / s[:, 2:]).astype(np.float32)
    k = int(round(outliers * n))
    if k:
        dst[r.choice(n, k, replace=False)] = r.uniform(0, 2048, (k, 2)).astype(np.float32)
    return src, dst


def host_ms(src, dst, model, **kw):
    """(best wall-clock ms, inliers, hypotheses) of vp_estimate_model_host"""
    nine, count, taken = np.empty(9), C.c_int(), C.c_int()
    best = None
    for _ in range(args.host_runs):
        t0 = time.perf_counter()
        _vp.check(_vp.lib().vp_estimate_model_host(src.ctypes.data, dst.ctypes.data, len(src), feature.MOTION_MODELS[model], kw.get("threshold", 3.0),
                                                   kw.get("max_iters", 2000), kw.get("confidence", 0.99), 0, nine.ctypes.data, None, C.addressof(count),
                                                   C.addressof(taken)))
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return round(best, 4), count.value, taken.value


def texture(shift, W=1920, H=1080):
    r = np.random.default_rng(5)
    k = 48
    fx, fy, ph, am = r.uniform(-0.6, 0.6, k), r.uniform(-0.6, 0.6, k), r.uniform(0, 2 * np.pi, k), r.uniform(0.5, 1.0, k)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    x, y = x - shift[0], y - shift[1]
    v = sum(a * np.cos(u * x + q * y + p) for a, u, q, p in zip(am, fx, fy, ph))
    return np.rint(np.clip(v / am.sum() * 1.5 + 0.5, 0, 1) * 255).astype(np.uint8)


def track_yardstick():
    a, b = DeviceMat.from_host(ctx, texture((0, 0))), DeviceMat.from_host(ctx, texture((2.3, -1.6)))
    corners = feature.good_features_to_track(a, 1000, 0.01, 5).reshape(-1, 2)
    pts = np.ascontiguousarray(np.resize(corners, (1000, 2)))
    pa, pb = feature.FlowPyramid(a, 3, (21, 21)), feature.FlowPyramid(b, 3, (21, 21))
    return median_ms(lambda: feature.track_points(pa, pb, pts))[0]


def main():
    first = track_yardstick()
    rows = []
    for model in MODELS:
        for n in (100, 1000, 10000, 100000):
            for share in (0.0, 0.3, 0.6):
                src, dst = pairs(n, model, share)
                M, inl = feature.estimate_motion(src, dst, model)
                row = {"model": model, "points": n, "outliers": share, "inliers": 0 if inl is None else int(inl.sum())}
                row["ms"], row["spread_ms"] = median_ms(lambda: feature.estimate_motion(src, dst, model))
                row["host_ms"], host_inliers, row["hypotheses"] = host_ms(src, dst, model)
                row["same_inliers_as_host"] = host_inliers == row["inliers"]
                rows.append(row)
    rounds = []
    for model in MODELS:
        for n in (1000, 100000):
            # nine pairs in ten are noise: 0.999999 cannot be reached within 512 hypotheses, every round counts
            src, dst = pairs(n, model, 0.9, 3)
            one = median_ms(lambda: feature.estimate_motion(src, dst, model, max_iters=256, confidence=0.999999))[0]
            two = median_ms(lambda: feature.estimate_motion(src, dst, model, max_iters=512, confidence=0.999999))[0]
            src, dst = pairs(n, model, 0.0, 4)
            short = median_ms(lambda: feature.estimate_motion(src, dst, model, max_iters=256))[0]
            full = median_ms(lambda: feature.estimate_motion(src, dst, model, max_iters=2000))[0]
            rounds.append({"model": model, "points": n, "one_round_ms": one, "two_rounds_ms": two, "further_round_ms": round(two - one, 5),
                           "stops_in_round_1_of_1_ms": short, "stops_in_round_1_of_8_ms": full, "idle_round_ms": round((full - short) / 7, 5)})
    second = track_yardstick()
    print(json.dumps({"iters": args.iters, "regions": args.regions, "host_runs": args.host_runs, "track_points_1000_ms": [first, second], "rows": rows,
                      "rounds": rounds}), flush=True)


if __name__ == "__main__":
    main()
