"""Times the contour-geometry pass (vision.utils.feature.contour_geometry -> vp_contour_geometry_i32) on the contours of 1080p masks.

    python tools/exp_geometry.py [--iters N] [--regions R] [--host-contours K]

One process, one GPU.  Every device figure is the median over R regions of N back-to-back calls, each region bracketed by HIP events on
the context's stream; a call uploads the point block, runs the one launch, copies the rows back and finishes them on the host.  One
JSON line.  Cases: the contours (RETR_LIST, CHAIN_APPROX_SIMPLE) of the S1 threshold mask and of 2 % and 10 % speckle.  In the same run,
the host loop the pass replaces - cv2_facade.minAreaRect (vp_min_area_rect_i32), cv2_facade.arcLength and cv2_facade.convexHull per
contour from a Python `for` - by wall clock over the first K contours of the list, scaled to the whole list (the loop is linear in the
contours).  Yardsticks of the same run: find_contours of the same mask and component_moments of its labels."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--regions", type=int, default=7)
ap.add_argument("--host-contours", type=int, default=4000)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cuauv-vision-pipeline_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (shares the HIP runtime with libvp)

import frames as F  # noqa: E402
from vision import _vp  # noqa: E402
from vision import cv2_facade as cv  # noqa: E402
from vision.devmat import DeviceMat  # noqa: E402
from vision.utils import feature  # noqa: E402

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
    return round(statistics.median(t), 5)


def host_loop_ms(contours):
    k = min(len(contours), args.host_contours)
    if k == 0:
        return 0.0, 0
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        for i in range(k):
            c = contours[i]
            cv.minAreaRect(c)
            cv.arcLength(c, True)
            cv.convexHull(c)
        t.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(t) * len(contours) / k, 3), k


def main():
    bgr = F.s1_buoy(0, W, H)
    rng = np.random.default_rng(7)
    masks = [("S1 mask", cv.inRange(cv.cvtColor(DeviceMat.from_host(ctx, bgr), cv.COLOR_BGR2LAB), (0, 150, 0), (255, 255, 255)))]
    for pct in (2, 10):
        masks.append((f"{pct} % speckle", DeviceMat.from_host(ctx, ((rng.random((H, W)) < pct / 100) * 255).astype(np.uint8))))
    rows = []
    for name, m in masks:
        cs = feature.find_contours(m, _vp.RETR_LIST, _vp.CHAIN_APPROX_SIMPLE)
        table = feature.contour_geometry(cs)
        n, labels, _, _ = feature.connected_components(m, max_labels=1 << 20)
        host_ms, timed = host_loop_ms(cs)
        r = {"case": name, "contours": len(cs), "points": int(len(cs._flat)), "rows_finished_by_host": int(np.count_nonzero(table["status"])),
             "geometry_ms": median_ms(lambda: feature.contour_geometry(cs)),
             "host_loop_ms": host_ms, "host_loop_contours_timed": timed,
             "find_contours_ms": median_ms(lambda: feature.find_contours(m, _vp.RETR_LIST, _vp.CHAIN_APPROX_SIMPLE)),
             "component_moments_ms": median_ms(lambda: feature.component_moments(labels, n))}
        r["host_loop_over_geometry"] = round(r["host_loop_ms"] / r["geometry_ms"], 1) if r["geometry_ms"] else None
        rows.append(r)
    print(json.dumps({"image": [H, W], "iters": args.iters, "regions": args.regions, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
