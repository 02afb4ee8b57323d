"""Times semi-global matching (vp_stereo_sgm_dev) on one 1280 x 720 device pair, the reference's HD720.

    python tools/exp_sgm.py [--iters N] [--regions R]

One process, one GPU.  Every device figure is the median over R regions of N back-to-back calls, each region bracketed by HIP events on
the context's stream and ended by a synchronise: whole calls, launches included.  Rows: num_disparities 64 / 128 x paths 4 / 8 at
block_size 5, `disparity_sgm` and `stereo_planes_sgm` (the Python layer on DeviceMats, nothing leaving HBM).  The three kernel groups -
cost volume, path aggregation, selection - come from the context's per-kernel events (vp_profile_begin / _end), the median over R
profiled calls; beside each time stand the bytes of C and S the group must move (computed from the shapes: C written once; every
direction reads C, reads S but for the first, writes S; the selection reads S and, with the left-right check, its diagonal) and the
rate that makes.  Yardsticks in the same run: `disparity` (block matching) at n = 64 and block_size 15, vp_stereo_sgm_host on one core
(one call, host clock, n = 64, 8 paths) and the 3 x 3 one-pass GaussianBlur.  The result at n = 64 with 8 paths is compared with
vp_stereo_sgm_host's.  One table, then one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--regions", type=int, default=5)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cuauv-vision-pipeline_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (shares the HIP runtime with libvp)

from vision import _vp  # noqa: E402
from vision.devmat import DeviceMat  # noqa: E402
from vision.utils import stereo  # noqa: E402

ctx = _vp.default_context()
lib = _vp.lib()
W, H = 1280, 720
FOCAL, BASELINE = 534.48, 0.12
BLOCK = 5


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


def groups_ms(fn):
    """median of the per-kernel event times of one profiled call, by group"""
    seen = {"k_sgm_cost": [], "k_sgm_path": [], "k_sgm_select": []}
    for _ in range(args.regions):
        ctx.profile_begin(64)
        fn()
        prof = ctx.profile_end()
        for k in seen:
            seen[k].append(prof[k][0])
    return {k: round(statistics.median(v), 5) for k, v in seen.items()}


def pair():
    rng = np.random.default_rng(21)
    a = rng.integers(0, 256, (H + 2, W + 40 + 2)).astype(np.int32)
    base = (sum(a[i:i + H, j:j + W + 40] for i in range(3) for j in range(3)) // 9).astype(np.uint8)
    return np.ascontiguousarray(base[:, :W]), np.ascontiguousarray(base[:, 40:40 + W])       # disparity 40 everywhere


def main():
    left, right = pair()
    dl, dr = DeviceMat.from_host(ctx, left), DeviceMat.from_host(ctx, right)
    disp = DeviceMat(ctx, (H, W), np.int16)
    blurred = DeviceMat(ctx, (H, W), np.uint8)

    def gauss():
        _vp.check(lib.vp_gaussian_blur_dev(ctx.handle, dl.dev_ptr, W, W, H, 1, 3, 3, 0.0, 0.0, blurred.dev_ptr), ctx.handle)

    host_out = np.empty((H, W), np.int16)
    p1, p2 = 8 * BLOCK * BLOCK, 32 * BLOCK * BLOCK
    t0 = time.perf_counter()
    _vp.check(lib.vp_stereo_sgm_host(left.ctypes.data, W, right.ctypes.data, W, W, H, 64, BLOCK, 0, 31, p1, p2, 10, 1, 8, host_out.ctypes.data, 2 * W))
    host_ms = (time.perf_counter() - t0) * 1e3
    yard = {"gaussian_3x3_ms": median_ms(gauss)[0], "stereo_sgm_host_one_core_n64_p8_ms": round(host_ms, 1),
            "disparity_bm_n64_b15_ms": median_ms(lambda: stereo.disparity(dl, dr, num_disparities=64, block_size=15))[0]}

    rows = []
    for n in (64, 128):
        x, y, cw, ch = stereo.valid_rect_sgm(W, H, n, BLOCK)
        vol = cw * ch * n * 2                                       # bytes of C, and of S
        for paths in (4, 8):
            def sgm():
                _vp.check(lib.vp_stereo_sgm_dev(ctx.handle, dl.dev_ptr, W, dr.dev_ptr, W, W, H, n, BLOCK, 0, 31, p1, p2, 10, 1, paths, disp.dev_ptr, 2 * W), ctx.handle)
            ms, spread = median_ms(sgm)
            g = groups_ms(sgm)
            moved = {"k_sgm_cost": vol, "k_sgm_path": vol * (3 * paths - 1), "k_sgm_select": 2 * vol}
            row = {"n": n, "paths": paths, "sgm_dev_ms": ms, "sgm_dev_spread_ms": spread, "volume_mb": round(vol / 1e6, 1)}
            for k, short in (("k_sgm_cost", "cost"), ("k_sgm_path", "paths"), ("k_sgm_select", "select")):
                row[short + "_ms"] = g[k]
                row[short + "_mb"] = round(moved[k] / 1e6, 1)
                row[short + "_gb_per_s"] = round(moved[k] / (g[k] * 1e-3) / 1e9, 1)
            row["disparity_sgm_ms"] = median_ms(lambda: stereo.disparity_sgm(dl, dr, num_disparities=n, paths=paths))[0]
            row["stereo_planes_sgm_ms"] = median_ms(lambda: stereo.stereo_planes_sgm(dl, dr, FOCAL, BASELINE, num_disparities=n, paths=paths))[0]
            sgm()
            got = disp.host_copy()
            row["answered"] = round(float((got != -16).mean()), 3)
            if (n, paths) == (64, 8):
                row["equals_host"] = bool(np.array_equal(got, host_out))
            rows.append(row)
    yard["gaussian_3x3_after_ms"] = median_ms(gauss)[0]
    print("%4s %5s %10s %8s %9s %9s %9s %11s %12s %10s %9s" % ("n", "paths", "sgm_dev ms", "spread", "cost ms", "paths ms", "select ms", "paths GB/s", "disparity ms",
                                                               "planes ms", "answered"))
    for r in rows:
        print("%4d %5d %10.4f %8.4f %9.4f %9.4f %9.4f %11.1f %12.4f %10.4f %9.3f" % (r["n"], r["paths"], r["sgm_dev_ms"], r["sgm_dev_spread_ms"], r["cost_ms"], r["paths_ms"],
                                                                                   r["select_ms"], r["paths_gb_per_s"], r["disparity_sgm_ms"], r["stereo_planes_sgm_ms"],
                                                                                   r["answered"]))
    for k, v in yard.items():
        print("%-40s %10.4f" % (k, v))
    print(json.dumps({"image": [H, W], "block_size": BLOCK, "iters": args.iters, "regions": args.regions, "yardsticks": yard, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
