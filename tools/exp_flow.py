"""Times pyramidal Lucas-Kanade tracking (FlowPyramid, track_points; libvp vp_lk_flow_dev) on two 1080p single-channel device images.

    python tools/exp_flow.py [--iters N] [--regions R]

One process, one GPU.  Every figure is the median over R regions of N back-to-back calls, each region bracketed by HIP events on the
context's stream.  One JSON line.  The pyramid build alone (three pyrDown launches); tracking alone over ready pyramids for 100, 1,000
and 10,000 points at 21 x 21 with four levels, with and without back_check (every call brings 16 bytes per point back, so every call
synchronises); the whole track_points call from two device images (both pyramids built inside).  The second frame is the first one
sampled 2.3 pixels to the right and 1.6 up, the points are the strongest corners of the first, repeated to the count.  Yardsticks in
the same run, before and after the cases: good_features_to_track, the pyrDown chain, and the 3 x 3 one-pass GaussianBlur."""
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "cuauv-vision-pipeline_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (shares the HIP runtime with libvp)

from vision import _vp  # noqa: E402
from vision import cv2_facade as cv  # noqa: E402
from vision.devmat import DeviceMat  # noqa: E402
from vision.utils import feature, transform  # noqa: E402

ctx = _vp.default_context()
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
    return round(statistics.median(t), 5), round(max(t) - min(t), 5)


def texture(shift):
    r = np.random.default_rng(5)
    k = 48
    fx, fy, ph, am = r.uniform(-0.6, 0.6, k), r.uniform(-0.6, 0.6, k), r.uniform(0, 2 * np.pi, k), r.uniform(0.5, 1.0, k)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    x, y = x - shift[0], y - shift[1]
    v = sum(a * np.cos(u * x + q * y + p) for a, u, q, p in zip(am, fx, fy, ph))
    return np.rint(np.clip(v / am.sum() * 1.5 + 0.5, 0, 1) * 255).astype(np.uint8)


def main():
    a, b = DeviceMat.from_host(ctx, texture((0, 0))), DeviceMat.from_host(ctx, texture((2.3, -1.6)))

    def yard():
        return {"good_features_ms": median_ms(lambda: feature.good_features_to_track(a, 1000, 0.01, 10))[0],
                "pyr_down_chain_ms": median_ms(lambda: transform.build_pyramid(a, 3))[0],
                "gaussian_3x3_ms": median_ms(lambda: cv.GaussianBlur(a, (3, 3), 0))[0]}

    first = yard()
    corners = feature.good_features_to_track(a, 10000, 0.01, 5).reshape(-1, 2)
    rows = [{"case": "FlowPyramid", "levels": 4}]
    rows[0]["ms"], rows[0]["spread_ms"] = median_ms(lambda: feature.FlowPyramid(a, 3, (21, 21)))
    pa, pb = feature.FlowPyramid(a, 3, (21, 21)), feature.FlowPyramid(b, 3, (21, 21))
    for n in (100, 1000, 10000):
        pts = np.ascontiguousarray(np.resize(corners, (n, 2)))
        found, status, _ = feature.track_points(pa, pb, pts)
        row = {"case": "track_points over pyramids", "points": n, "corners": int(min(n, len(corners))), "tracked": int(status.sum()),
               "median_shift": [round(float(v), 3) for v in np.median(found.reshape(-1, 2)[status] - pts[status], axis=0)]}
        row["ms"], row["spread_ms"] = median_ms(lambda: feature.track_points(pa, pb, pts))
        row["back_check_ms"] = median_ms(lambda: feature.track_points(pa, pb, pts, back_check=1.0))[0]
        rows.append(row)
    pts = np.ascontiguousarray(np.resize(corners, (1000, 2)))
    ms, spread = median_ms(lambda: feature.track_points(a, b, pts))
    rows.append({"case": "track_points from two device images", "points": 1000, "ms": ms, "spread_ms": spread})
    second = yard()
    print(json.dumps({"image": [H, W], "iters": args.iters, "regions": args.regions, "yardsticks_first": first, "yardsticks_second": second, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
