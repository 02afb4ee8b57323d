"""Times robust rigid motion (vp_fit_rigid_* through vision.utils.stereo) on seeded point pairs and on one 1280 x 720 synthetic rig.

    python tools/exp_rigid.py [--iters N] [--regions R]

One process, one GPU.  Every figure is the median over R regions of N back-to-back calls, each region bracketed by HIP events on the
context's stream and ended by a synchronise: whole synchronised calls, launches and the host arrays' staging included.  Rows:
fit_rigid at 1,000 / 10,000 / 100,000 / 1,000,000 pairs with 0 / 30 / 60 % gross outliers under both metrics; rigid_from_tracks on
1280 x 720 device point images with 1,000 and 10,000 tracks; StereoRig.ego_motion from two disparity images.  Yardsticks in the same
run: fit_plane on a full frame, estimate_motion (affine, 100,000 pairs), vp_reproject_to_3d_dev, and vp_fit_rigid_host on one core
for 100,000 pairs.  One table, then one JSON line."""
import argparse
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
import rigid_cases  # noqa: E402
from vision import _vp  # noqa: E402
from vision.devmat import DeviceMat  # noqa: E402
from vision.utils import feature, stereo  # noqa: E402

ctx = _vp.default_context()
lib = _vp.lib()
W, H = 1280, 720
F, B = 700.0, 0.12
SIGMA = 0.003


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


def scene_depth(Rm, t):
    """Z (H, W) of a slanted plane, given in the first frame, after the motion (Rm, t), along every pixel's ray"""
    x, y = np.meshgrid((np.arange(W) - W / 2) / F, (np.arange(H) - H / 2) / F)
    rays = np.stack([x, y, np.ones_like(x)], 2)
    n, d = np.array([0.1, -0.05, -1.0]), 2.0
    nn = Rm @ n
    return (nn @ t - d) / (rays @ nn), rays


def main():
    rows = []

    def row(name, fn, fit=None):
        ms, spread = median_ms(fn)
        r = {"row": name, "ms": ms, "spread_ms": spread}
        if fit is not None:
            r.update(found=fit.found, usable=fit.n_usable, inliers=fit.n_inliers, hypotheses=fit.n_hypotheses)
        rows.append(r)

    for n in (1000, 10000, 100000, 1000000):
        for share in (0.0, 0.3, 0.6):
            src, dst, _ = rigid_cases.pairs(n, [rigid_cases.MOTION_1], [1], SIGMA, share, 7)
            for name, kw in (("euclid", dict(threshold=4 * SIGMA)), ("disparity", dict(threshold=1.0, camera=(F, B)))):
                row("fit_rigid_%d_out%d_%s" % (n, round(100 * share), name), lambda: stereo.fit_rigid(src, dst, **kw), stereo.fit_rigid(src, dst, **kw))
    # two frames of one plane seen by a rig, the tracks from the geometry
    Rm, t = rigid_cases.rotation(0.02, -0.04, 0.03), np.array([0.05, -0.02, 0.08])
    z0, rays = scene_depth(np.eye(3), np.zeros(3))
    z1, _ = scene_depth(Rm, t)
    disp = [DeviceMat.from_host(ctx, np.rint(F * B / z * 16).astype(np.int16)) for z in (z0, z1)]
    rig = stereo.StereoRig(np.array([[F, 0, W / 2], [0, F, H / 2], [0, 0, 1]]), np.zeros(5), np.array([[F, 0, W / 2], [0, F, H / 2], [0, 0, 1]]), np.zeros(5), (W, H),
                           np.eye(3), [-B, 0.0, 0.0])
    pts = [rig.points(d) for d in disp]
    r = np.random.default_rng(3)
    for n in (1000, 10000):
        px = np.stack([r.integers(0, W, n), r.integers(0, H, n)], 1)
        c1 = (z0[px[:, 1], px[:, 0], None] * rays[px[:, 1], px[:, 0]]) @ Rm.T + t
        nxt = np.stack([rig.focal_px * c1[:, 0] / c1[:, 2] + rig.cx, rig.focal_px * c1[:, 1] / c1[:, 2] + rig.cy], 1).astype(np.float32)
        prev = px.astype(np.float32)
        kw = dict(threshold=1.0, camera=(rig.focal_px, rig.baseline_m))
        row("rigid_from_tracks_%d" % n, lambda: stereo.rigid_from_tracks(pts[0], pts[1], prev, nxt, **kw), stereo.rigid_from_tracks(pts[0], pts[1], prev, nxt, **kw))
    row("rig_ego_motion_10000", lambda: rig.ego_motion(disp[0], disp[1], prev, nxt), rig.ego_motion(disp[0], disp[1], prev, nxt))
    # yardsticks
    pkw = dict(threshold=0.012, max_iters=1000)
    row("fit_plane_full", lambda: stereo.fit_plane(pts[0], **pkw))
    src2, dst2, _, _ = model_restate.make_pairs(100000, model_restate.AFFINE, 0.3)
    row("estimate_motion_affine_100k", lambda: feature.estimate_motion(src2, dst2, "affine"))
    xyz = DeviceMat(ctx, (H, W, 3), np.float32)
    q = np.ascontiguousarray(rig.Q)
    row("reproject_to_3d_dev", lambda: _vp.check(lib.vp_reproject_to_3d_dev(ctx.handle, disp[0].dev_ptr, 2 * W, 0, W, H, q.ctypes.data, -16, xyz.dev_ptr, 12 * W), ctx.handle))
    src, dst, _ = rigid_cases.pairs(100000, [rigid_cases.MOTION_1], [1], SIGMA, 0.3, 7)
    result, counts = np.zeros(_vp.RIGID_RESULT), np.zeros(4, np.int32)
    t0 = time.perf_counter()
    _vp.check(lib.vp_fit_rigid_host(src.ctypes.data, dst.ctypes.data, len(src), 0, 4 * SIGMA, 0.0, 0.0, 1000, 0.99, 0, None, result.ctypes.data, counts.ctypes.data))
    rows.append({"row": "fit_rigid_host_one_core_100000_out30_euclid", "ms": round((time.perf_counter() - t0) * 1e3, 2), "spread_ms": 0.0, "usable": int(counts[0]),
                 "inliers": int(counts[1]), "hypotheses": int(counts[2])})
    print("%-44s %10s %10s %9s %9s %6s" % ("row", "ms", "spread", "usable", "inliers", "hyp"))
    for r_ in rows:
        print("%-44s %10.4f %10.4f %9s %9s %6s" % (r_["row"], r_["ms"], r_["spread_ms"], r_.get("usable", ""), r_.get("inliers", ""), r_.get("hypotheses", "")))
    print(json.dumps({"image": [H, W], "iters": args.iters, "regions": args.regions, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
