"""cv2.findContours of ONE 1080p device image with RETR_TREE (its hierarchy) against RETR_EXTERNAL, on the S1 threshold mask and on
2 % / 10 % speckle: ms per call (device image in, contours and hierarchy out), medians of `calls`, the two modes alternated.
usage: python tools/exp_contour_tree.py [calls]        (json on the last line)"""
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
from vision.utils import color, feature


def measure(calls=200):
    ctx = _vp.default_context()
    g = color.bgr_to_gray(F.s3_noise(0))[0]
    masks = [("s1_threshold_mask", color.range_threshold(color.bgr_to_lab(F.s1_buoy(0))[1][1], 150, 255)),
             ("s3_noise_2pct", color.range_threshold(g, 230, 255)), ("s3_noise_10pct", color.range_threshold(g, 190, 255))]
    out = {}
    for name, m in masks:
        m = DeviceMat.from_host(ctx, np.ascontiguousarray(np.asarray(m)), binary=True)
        cs = feature.outer_contours(m)
        tree = feature.find_contours(m, _vp.RETR_TREE, _vp.CHAIN_APPROX_SIMPLE, with_hierarchy=True)[0]
        n = max(10, calls // (1 + len(tree) // 2000))
        t_ext, t_tree = [], []
        for _ in range(n):
            t0 = time.perf_counter()
            feature.outer_contours(m)
            t1 = time.perf_counter()
            feature.find_contours(m, _vp.RETR_TREE, _vp.CHAIN_APPROX_SIMPLE, with_hierarchy=True)
            t2 = time.perf_counter()
            t_ext.append(t1 - t0)
            t_tree.append(t2 - t1)
        out[name] = {"external_ms": round(1e3 * float(np.median(t_ext)), 4), "tree_ms": round(1e3 * float(np.median(t_tree)), 4),
                     "external_contours": len(cs), "tree_contours": len(tree), "calls": n}
    return out


if __name__ == "__main__":
    r = measure(int(sys.argv[1]) if len(sys.argv) > 1 else 200)
    for k, v in r.items():
        print(k, v)
    print(json.dumps(r))
