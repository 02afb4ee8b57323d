"""Times robust plane fitting (vp_fit_plane_dev through vision.utils.stereo) on one 1280 x 720 stereo pair of the synthetic scenes of
tests/stereo_cases.py (two fronto-parallel planes, disparities 5 and 11), beside the stereo stack's other tails.

    python tools/exp_plane.py [--iters N] [--regions R]

One process, one GPU.  Every figure is the median over R regions of N back-to-back calls, each region bracketed by HIP events on the
context's stream and ended by a synchronise: whole synchronised calls, launches included.  Rows: fit_plane on the metric points of
the matched pair, full frame and a 200 x 200 box; fit_plane on a full frame of one exact plane with 30 % and with 60 % of the pixels
replaced by gross outliers; fit_planes(k=3); StereoRig.fit_plane from the disparity image (disparity space).  Yardsticks in the
same run: normals_from_depth, vp_reproject_to_3d_dev, estimate_motion (affine, 100,000 pairs), and vp_fit_plane_host on one core
for the full-frame row.  One table, then one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--regions", type=int, default=5)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cuauv-vision-pipeline_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (shares the HIP runtime with libvp)

import model_restate  # noqa: E402
import stereo_cases  # noqa: E402
from vision import _vp  # noqa: E402
from vision.devmat import DeviceMat  # noqa: E402
from vision.utils import feature, stereo  # noqa: E402

ctx = _vp.default_context()
lib = _vp.lib()
W, H = 1280, 720


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


def exact_plane(outliers, seed):
    """a full frame of one slanted plane in metres, the share `outliers` of its pixels at a random depth"""
    r = np.random.default_rng(seed)
    x, y = np.meshgrid((np.arange(W) - W / 2) / 700.0, (np.arange(H) - H / 2) / 700.0)
    z = 2.0 + 0.3 * x - 0.2 * y + r.normal(0, 0.003, (H, W))
    bad = r.random((H, W)) < outliers
    z[bad] = r.uniform(0.5, 5.0, int(bad.sum()))
    return np.stack([x * z, y * z, z], -1).astype(np.float32)


def main():
    rig = stereo.StereoRig(np.array([[700.0, 0, 640], [0, 700.0, 360], [0, 0, 1]]), np.zeros(5), np.array([[700.0, 0, 640], [0, 700.0, 360], [0, 0, 1]]), np.zeros(5),
                           (W, H), np.eye(3), [-0.12, 0.0, 0.0])
    left, right = stereo_cases.two_plane_pair(H, W, seed=3)
    disp = stereo.disparity(DeviceMat.from_host(ctx, left), DeviceMat.from_host(ctx, right), num_disparities=16, block_size=15)
    pts = rig.points(disp)
    depth = stereo.depth_from_disparity(disp, rig.focal_px, rig.baseline_m)
    rows = []

    def row(name, fn, fit=None):
        ms, spread = median_ms(fn)
        r = {"row": name, "ms": ms, "spread_ms": spread}
        if fit is not None:
            r.update(found=fit.found, usable=fit.usable, inliers=fit.inliers, hypotheses=fit.hypotheses)
        rows.append(r)

    kw = dict(threshold=0.05, max_iters=1000)
    row("fit_plane_full", lambda: stereo.fit_plane(pts, **kw), stereo.fit_plane(pts, **kw))
    box = (W // 2 + 100, 200, 200, 200)
    row("fit_plane_box_200", lambda: stereo.fit_plane(pts, box=box, **kw), stereo.fit_plane(pts, box=box, **kw))
    for share in (0.3, 0.6):
        p = DeviceMat.from_host(ctx, exact_plane(share, 5))
        k2 = dict(threshold=0.012, max_iters=1000)
        row("fit_plane_outliers_%d" % round(100 * share), lambda: stereo.fit_plane(p, **k2), stereo.fit_plane(p, **k2))
    row("fit_planes_k3", lambda: stereo.fit_planes(pts, 3, 1000, **kw))
    row("rig_fit_plane_disparity", lambda: rig.fit_plane(disp, threshold=0.5, max_iters=1000), rig.fit_plane(disp, threshold=0.5, max_iters=1000))
    # yardsticks
    row("normals_from_depth", lambda: stereo.normals_from_depth(depth, rig.focal_px, rig.cx, rig.cy))
    xyz = DeviceMat(ctx, (H, W, 3), np.float32)
    q = np.ascontiguousarray(rig.Q)
    row("reproject_to_3d_dev", lambda: _vp.check(lib.vp_reproject_to_3d_dev(ctx.handle, disp.dev_ptr, 2 * W, 0, W, H, q.ctypes.data, -16, xyz.dev_ptr, 12 * W), ctx.handle))
    src, dst, _, _ = model_restate.make_pairs(100000, model_restate.AFFINE, 0.3)
    row("estimate_motion_affine_100k", lambda: feature.estimate_motion(src, dst, "affine"))
    host = pts.host_copy()
    result, counts = np.zeros(12), np.zeros(4, np.int32)
    t0 = time.perf_counter()
    _vp.check(lib.vp_fit_plane_host(host.ctypes.data, 12 * W, W, H, None, None, 0, 0, kw["threshold"], kw["max_iters"], 0.99, 0, None, 0, result.ctypes.data, counts.ctypes.data))
    rows.append({"row": "fit_plane_host_one_core_full", "ms": round((time.perf_counter() - t0) * 1e3, 2), "spread_ms": 0.0, "usable": int(counts[0]),
                 "inliers": int(counts[1]), "hypotheses": int(counts[2])})
    print("%-30s %10s %10s %9s %9s %6s" % ("row", "ms", "spread", "usable", "inliers", "hyp"))
    for r in rows:
        print("%-30s %10.4f %10.4f %9s %9s %6s" % (r["row"], r["ms"], r["spread_ms"], r.get("usable", ""), r.get("inliers", ""), r.get("hypotheses", "")))
    print(json.dumps({"image": [H, W], "iters": args.iters, "regions": args.regions, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
