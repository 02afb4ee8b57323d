"""Times the features over a scale pyramid (vision.utils.feature.pyramid_features, vision.utils.sift.PyramidSIFT; libvp
vp_pyr_features_*).

    python tools/exp_pyr_features.py [--iters N] [--regions R]

One process, one GPU.  Every figure is the median over R regions of N back-to-back calls, each region bracketed by HIP events on the
context's stream; every call is whole and synchronised (results come back as host arrays).  One JSON line.  On one 1080p device
image (the sum of cosines of tools/exp_features.py): pyramid_features at threshold 20 for levels 1 / 4 / 8 and budgets of 500 / 2,000 /
10,000 points, with the points found per level; as the yardstick, the same result composed level by level from the existing entries
(resize from the level before, fast_corners capped at the level's quota, describe_points - one host round trip per level);
PyramidSIFT.match end to end on the image against a 256 x 256 crop of it, shown at its own size and enlarged to twice it, as the
sources, beside the single-scale SIFT.match on the same sources."""
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
from vision.utils import feature  # noqa: E402
from vision.utils.sift import SIFT, PyramidSIFT  # noqa: E402

ctx = _vp.default_context()
THRESHOLD = 20


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


def quotas(sizes, n):
    areas = [w * h for w, h in sizes]
    q = [0] + [n * a // sum(areas) for a in areas[1:]]
    q[0] = n - sum(q)
    return q


def composed(dev, levels, budget):
    """the yardstick: level by level through the entries that were there before (the describable-region restriction is left out:
    describe_points drops the corners near the border after the cap, so a level may keep a few less)"""
    sizes = feature.pyramid_level_sizes(dev.shape[1], dev.shape[0], levels)
    found, level = 0, dev
    for (w, h), q in zip(sizes, quotas(sizes, budget)):
        if level.shape != (h, w):
            level = cv.resize(level, (w, h))
        pts, _ = feature.fast_corners(level, THRESHOLD, True, q)
        found += len(feature.describe_points(level, pts)[0])
    return found


def main():
    host = texture()
    dev = DeviceMat.from_host(ctx, host)
    res = {"iters": args.iters, "regions": args.regions, "threshold": THRESHOLD, "pyramid": [], "composed": []}
    for levels in (1, 4, 8):
        for budget in (500, 2000, 10000):
            out = feature.pyramid_features(dev, THRESHOLD, budget, levels)
            ms, spread = median_ms(lambda: feature.pyramid_features(dev, THRESHOLD, budget, levels))
            res["pyramid"].append({"levels": levels, "budget": budget, "points": len(out[0]), "per_level": np.bincount(out[2], minlength=levels).tolist(), "ms": ms,
                                   "spread_ms": spread})
            n = composed(dev, levels, budget)
            ms, spread = median_ms(lambda: composed(dev, levels, budget))
            res["composed"].append({"levels": levels, "budget": budget, "points": n, "ms": ms, "spread_ms": spread})
    crop = np.ascontiguousarray(host[400:656, 800:1056])
    res["match"] = []
    for name, cls in (("PyramidSIFT", PyramidSIFT), ("SIFT", SIFT)):
        s = cls()
        s.add_many(same=crop, twice=np.ascontiguousarray(cv.resize(crop, (512, 512))))
        matched, fkp, _ = s.match(dev)
        ms, spread = median_ms(lambda: s.match(dev))
        res["match"].append({"class": name, "frame_keypoints": len(fkp), "found": [m[0] for m in matched], "good": [len(m[1]) for m in matched],
                             "inliers": [int(sum(m[3])) for m in matched], "ms": ms, "spread_ms": spread})
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
