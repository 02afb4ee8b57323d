"""Times stereo block matching (vp_stereo_bm_dev, vp_depth_from_disparity_dev) on one 1280 x 720 device pair, the reference's HD720.

    python tools/exp_stereo.py [--iters N] [--regions R]

One process, one GPU.  Every device figure is the median over R regions of N back-to-back calls, each region bracketed by HIP events on
the context's stream and ended by a synchronise: whole calls, launches included.  Rows: num_disparities 64 / 128 x block_size 9 / 15 /
21, `disparity` and `stereo_depth` (the Python layer on DeviceMats, the disparity never leaving HBM), and the absolute differences per
second the matcher's time stands for, w h n per pair counted once.  Yardsticks in the same run: vp_stereo_bm_host on one core (one
call, host clock, at n = 64 and block_size = 15), matchTemplate TM_CCORR with a 16 x 16 template and the 3 x 3 one-pass GaussianBlur on
the left image.  The result of every configuration is compared with vp_stereo_bm_host's once where that is computed.  One table, then
one JSON line."""
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
    score = DeviceMat(ctx, (H - 15, W - 15), np.float32)
    templ = DeviceMat.from_host(ctx, np.ascontiguousarray(left[300:316, 700:716]))

    def gauss():
        _vp.check(lib.vp_gaussian_blur_dev(ctx.handle, dl.dev_ptr, W, W, H, 1, 3, 3, 0.0, 0.0, blurred.dev_ptr), ctx.handle)

    def ccorr():
        _vp.check(lib.vp_match_template_dev(ctx.handle, dl.dev_ptr, W, W, H, 1, templ.dev_ptr, 16, 16, 16, _vp.TM_CCORR, score.dev_ptr, (W - 15) * 4), ctx.handle)

    host_out = np.empty((H, W), np.int16)
    t0 = time.perf_counter()
    _vp.check(lib.vp_stereo_bm_host(left.ctypes.data, W, right.ctypes.data, W, W, H, 64, 15, 0, 31, 10, 15, host_out.ctypes.data, 2 * W))
    host_ms = (time.perf_counter() - t0) * 1e3
    yard = {"gaussian_3x3_ms": median_ms(gauss)[0], "match_template_ccorr_16_ms": median_ms(ccorr)[0], "stereo_bm_host_one_core_n64_b15_ms": round(host_ms, 1)}

    rows = []
    for n in (64, 128):
        for bs in (9, 15, 21):
            def bm():
                _vp.check(lib.vp_stereo_bm_dev(ctx.handle, dl.dev_ptr, W, dr.dev_ptr, W, W, H, n, bs, 0, 31, 10, 15, disp.dev_ptr, 2 * W), ctx.handle)
            bm_ms, spread = median_ms(bm)
            row = {"n": n, "block_size": bs, "bm_dev_ms": bm_ms, "bm_dev_spread_ms": spread, "gsad_per_s": round(W * H * n / (bm_ms * 1e-3) / 1e9, 2),
                   "disparity_ms": median_ms(lambda: stereo.disparity(dl, dr, num_disparities=n, block_size=bs))[0],
                   "stereo_depth_ms": median_ms(lambda: stereo.stereo_depth(dl, dr, FOCAL, BASELINE, num_disparities=n, block_size=bs))[0]}
            got = disp.host_copy()
            row["answered"] = round(float((got != -16).mean()), 3)
            if (n, bs) == (64, 15):
                row["equals_host"] = bool(np.array_equal(got, host_out))
            rows.append(row)
    yard["gaussian_3x3_after_ms"] = median_ms(gauss)[0]
    print("%4s %5s %10s %8s %12s %12s %15s %9s" % ("n", "block", "bm_dev ms", "spread", "G absdiff/s", "disparity ms", "stereo_depth ms", "answered"))
    for r in rows:
        print("%4d %5d %10.4f %8.4f %12.2f %12.4f %15.4f %9.3f" % (r["n"], r["block_size"], r["bm_dev_ms"], r["bm_dev_spread_ms"], r["gsad_per_s"], r["disparity_ms"],
                                                                 r["stereo_depth_ms"], r["answered"]))
    for k, v in yard.items():
        print("%-40s %10.4f" % (k, v))
    print(json.dumps({"image": [H, W], "iters": args.iters, "regions": args.regions, "yardsticks": yard, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
