"""Filling a contour in an image that lives on the device: `draw_contours(frame, [c], color, thickness=-1)` for the largest contour of
the S1 frame's mask in a 1080p BGR frame without a host copy.  Each run starts from such a frame and ends when the frame is valid on
the device again - for a tree that fills on the host this covers the download, the fill and the upload the next operator would make,
for one that fills on the device the kernels.  HIP events around the run (they bracket the host's share as well) and the wall clock,
synchronised at the end; median over the runs after warm-up.  Beside it: the outline (thickness=1) of the same contour, and, where the
tree has it, fill_ratio on device images against the same call on host images.
The file uses only entry points the tree had before the device fill existed, so it measures an older checkout unchanged.
usage: python tools/exp_fill.py [runs] [warmup]        (json on the last line)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "cuauv-vision-pipeline_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import frames as F
from vision import _vp
from vision.devmat import DeviceMat
from vision.utils import color, draw, feature


def _timed(ctx, make, fn, runs, warmup):
    ev, wall = [], []
    for k in range(warmup + runs):
        arg = make()
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.timer_start()
        fn(arg)
        ms = ctx.timer_stop()                        # (synchronises)
        dt = time.perf_counter() - t0
        if k >= warmup:
            ev.append(ms)
            wall.append(1e3 * dt)
    return {"event_ms": round(float(np.median(ev)), 4), "wall_ms": round(float(np.median(wall)), 4), "runs": runs}


def measure(runs=20, warmup=3):
    ctx = _vp.default_context()
    frame = F.s1_buoy(0)
    h, w = frame.shape[:2]
    mask = color.range_threshold(color.bgr_to_lab(frame)[1][1], 150, 255)
    contours = feature.outer_contours(mask)
    big = max(contours, key=feature.contour_area)
    pts = np.asarray(big).reshape(-1, 2)
    out = {"size": [w, h], "contour_points": int(len(pts)), "contour_rows": int(pts[:, 1].max() - pts[:, 1].min() + 1),
           "contour_area": float(feature.contour_area(big)), "device_fill": hasattr(draw, "_device_fill")}

    def fresh():
        return DeviceMat.from_host(ctx, frame)

    def draw_with(thickness):
        def fn(dev):
            draw.draw_contours(dev, [big], (0, 255, 0), thickness)
            dev.refresh_device(ctx)                  # where the draw went through the host: the upload the next operator makes
        return fn
    out["fill"] = _timed(ctx, fresh, draw_with(-1), runs, warmup)
    out["outline"] = _timed(ctx, fresh, draw_with(1), runs, warmup)
    if hasattr(feature, "fill_ratio"):
        host_mask = np.asarray(mask).copy()
        dev_mask = DeviceMat.from_host(ctx, host_mask, binary=True)
        out["fill_ratio_device"] = _timed(ctx, lambda: None, lambda _: feature.fill_ratio(dev_mask, big, dev_mask), runs, warmup)
        out["fill_ratio_host"] = _timed(ctx, lambda: None, lambda _: feature.fill_ratio(host_mask, big, host_mask), runs, warmup)
        out["fill_ratio_value"] = [float(feature.fill_ratio(dev_mask, big, dev_mask)), float(feature.fill_ratio(host_mask, big, host_mask))]
    return out


if __name__ == "__main__":
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    print(json.dumps(measure(runs, warmup)))
