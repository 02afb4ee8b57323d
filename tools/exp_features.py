"""Times the feature operators (vision.utils.feature fast_corners, describe_points, match_descriptors; vision.utils.sift.SIFT; libvp
vp_features.hip).

    python tools/exp_features.py [--iters N] [--regions R]

One process, one GPU.  Every figure is the median over R regions of N back-to-back calls, each region bracketed by HIP events on the
context's stream; every call is whole and synchronised (results come back as host arrays).  One JSON line.  On one 1080p device
image (a sum of cosines, so that there are corners at every scale of threshold): fast_corners at thresholds 10 / 20 / 40 with the
number of corners found; describe_points of 100 / 1,000 / 10,000 of them; match_descriptors (k = 2, host descriptors in, the upload
inside the call) at 500 x 500, 2,000 x 2,000, 10,000 x 10,000 and 100 x 100,000 with the plan's query tiles and train splits - the
last one exercises the split of the train set; SIFT.match end to end on the image against a 256 x 256 crop of it as the one source.
Yardsticks in the same run: good_features_to_track, the 3 x 3 one-pass GaussianBlur, estimate_motion (homography, 1,000 pairs)."""
import argparse
import ctypes as C
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
from vision.devmat import DeviceMat  # noqa: E402
from vision.utils import feature  # noqa: E402
from vision.utils.sift import SIFT  # noqa: E402

ctx = _vp.default_context()


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


def texture(W=1920, H=1080):
    r = np.random.default_rng(5)
    k = 48
    fx, fy, ph, am = r.uniform(-0.6, 0.6, k), r.uniform(-0.6, 0.6, k), r.uniform(0, 2 * np.pi, k), r.uniform(0.5, 1.0, k)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    v = sum(a * np.cos(u * x + q * y + p) for a, u, q, p in zip(am, fx, fy, ph))
    return np.rint(np.clip(v / am.sum() * 1.5 + 0.5, 0, 1) * 255).astype(np.uint8)


def blur_yardstick(dev):
    out = DeviceMat(ctx, dev.shape)
    ctx.set_option(_vp.OPT_BLUR_ONEPASS, 1)
    ms = median_ms(lambda: _vp.check(_vp.lib().vp_gaussian_blur_dev(ctx.handle, dev.dev_ptr, dev.shape[1], dev.shape[1], dev.shape[0], 1, 3, 3, 0.0, 0.0, out.dev_ptr),
                                     ctx.handle))[0]
    ctx.set_option(_vp.OPT_BLUR_ONEPASS, -1)
    return ms


def main():
    host = texture()
    dev = DeviceMat.from_host(ctx, host)
    res = {"iters": args.iters, "regions": args.regions}
    res["blur3_onepass_ms"] = [blur_yardstick(dev)]
    res["good_features_ms"] = median_ms(lambda: feature.good_features_to_track(dev, 1000, 0.01, 5))[0]
    res["fast"] = []
    for t in (10, 20, 40):
        pts, _ = feature.fast_corners(dev, t)
        ms, spread = median_ms(lambda: feature.fast_corners(dev, t))
        res["fast"].append({"threshold": t, "corners": len(pts), "ms": ms, "spread_ms": spread})
    r = np.random.default_rng(1)
    res["describe"] = []
    for n in (100, 1000, 10000):
        pts = np.stack([r.uniform(20, 1900, n), r.uniform(20, 1060, n)], axis=1).astype(np.float32)
        ms, spread = median_ms(lambda: feature.describe_points(dev, pts))
        res["describe"].append({"points": n, "ms": ms, "spread_ms": spread})
    res["match"] = []
    qt, sp = C.c_int(), C.c_int()
    for nq, nt in ((500, 500), (2000, 2000), (10000, 10000), (100, 100000)):
        q, tr = r.integers(0, 256, (nq, 32), dtype=np.uint8), r.integers(0, 256, (nt, 32), dtype=np.uint8)
        _vp.check(_vp.lib().vp_hamming_plan(nq, nt, 32, C.addressof(qt), C.addressof(sp)))
        ms, spread = median_ms(lambda: feature.match_descriptors(q, tr, 2))
        res["match"].append({"queries": nq, "train": nt, "query_tiles": qt.value, "train_splits": sp.value, "ms": ms, "spread_ms": spread,
                             "pairs_per_us": round(nq * nt / (ms * 1e3), 1)})
    s = SIFT()
    kp, _ = s.add_source("crop", np.ascontiguousarray(host[400:656, 800:1056]))
    matched, fkp, _ = s.match(dev)
    ms, spread = median_ms(lambda: s.match(dev))
    res["sift_match"] = {"source_keypoints": len(kp), "frame_keypoints": len(fkp), "found": [m[0] for m in matched], "good": [len(m[1]) for m in matched],
                         "inliers": [int(sum(m[3])) for m in matched], "ms": ms, "spread_ms": spread}
    src = r.uniform(0, 2048, (1000, 2)).astype(np.float32)
    dst = (src * 1.01 + (3.0, -2.0)).astype(np.float32)
    res["estimate_motion_homography_1000_ms"] = median_ms(lambda: feature.estimate_motion(src, dst, "homography"))[0]
    res["blur3_onepass_ms"].append(blur_yardstick(dev))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
