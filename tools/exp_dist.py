"""Times the distance operators (vp_distance_transform_dev, vp_min_max_loc_dev) on 1080p device images.

    python tools/exp_dist.py [--iters N] [--regions R]

One process, one GPU.  Every figure is the median over R regions of N back-to-back calls, each region bracketed by HIP events on the
context's stream.  One JSON line.  Masks (zero pixels are the sources): the Lab threshold mask of the S1 frame; speckle with 2 % and
10 % of the pixels non-zero, and the same with 2 % and 10 % zero; one zero pixel in a corner of an otherwise full frame, the longest
search; a frame without zeros.  Cases: DIST_L2 from bytes and from the bit plane on every mask; every metric and L1 as CV_8U on the S1
mask; minMaxLoc on the uint8 mask, on the float32 map and under the mask as bit plane; largest_inscribed_circle end to end (both
launches, the 32 bytes back, the Python layer).  A 1920 x 2304 frame (above the plan's switch: the column pass reads device memory) and
the same frame cut to 2048 rows (LDS strips) give the two forms of the column pass side by side.  Yardsticks, timed in the same run
before and after the cases: the 3x3 one-pass GaussianBlur, the labelling of the S1 mask from its bit plane (vp_ccl_bits_dev) and
countNonZero."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--regions", type=int, default=7)
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
lib = _vp.lib()
W, H = 1920, 1080


def median_ms(fn):
    for _ in range(3):
        fn()
    ctx.synchronize()
    t = []
    for _ in range(args.regions):
        ctx.timer_start()
        for _ in range(args.iters):
            fn()
        t.append(ctx.timer_stop() / args.iters)
    return round(statistics.median(t), 5)


def mask_of(img):
    """a known 0 / 255 device mask with its bit plane, as inRange leaves it"""
    m = cv.inRange(DeviceMat.from_host(ctx, img), 1, 255)
    assert m.bit_plane(ctx) is not None
    return m


def dist_case(mask, metric, depth, out, use_bits):
    h, w = mask.shape
    bits = mask.bit_plane(ctx).ptr if use_bits else None
    es = 1 if depth == _vp.DEPTH_8U else 4

    def fn():
        _vp.check(lib.vp_distance_transform_dev(ctx.handle, mask.dev_ptr, w, w, h, bits, metric, depth, out.dev_ptr, w * es), ctx.handle)
    return median_ms(fn)


def main():
    rng = np.random.default_rng(7)
    lab = cv.cvtColor(DeviceMat.from_host(ctx, F.s1_buoy(0, W, H)), cv.COLOR_BGR2LAB)
    s1 = cv.inRange(lab, (0, 150, 0), (255, 255, 255))
    assert s1.bit_plane(ctx) is not None
    noise = rng.random((H, W))
    corner = np.full((H, W), 255, np.uint8)
    corner[H - 1, 0] = 0
    masks = [("S1 threshold mask", s1)]
    for pct in (2, 10):
        masks.append(("speckle, %d %% non-zero" % pct, mask_of((noise < pct / 100.0).astype(np.uint8) * 255)))
        masks.append(("speckle, %d %% zero" % pct, mask_of((noise >= pct / 100.0).astype(np.uint8) * 255)))
    masks += [("one zero in a corner", mask_of(corner)), ("no zero", mask_of(np.full((H, W), 255, np.uint8)))]
    out32 = DeviceMat(ctx, (H, W), np.float32)
    out8 = DeviceMat(ctx, (H, W), np.uint8)
    blurred = DeviceMat(ctx, (H, W), np.uint8)
    grey = DeviceMat.from_host(ctx, rng.integers(0, 256, (H, W), dtype=np.uint8))

    def yard():
        def gauss():
            _vp.check(lib.vp_gaussian_blur_dev(ctx.handle, grey.dev_ptr, W, W, H, 1, 3, 3, 0.0, 0.0, blurred.dev_ptr), ctx.handle)
        return {"gaussian_3x3_ms": median_ms(gauss), "ccl_bits_s1_ms": median_ms(lambda: feature.connected_components(s1)),
                "count_nonzero_ms": median_ms(lambda: cv.countNonZero(s1))}

    first = yard()
    rows = []
    for name, m in masks:
        rows.append({"case": "DIST_L2", "mask": name, "zeros": H * W - cv.countNonZero(m), "bytes_ms": dist_case(m, _vp.DIST_L2, _vp.DEPTH_32F, out32, False),
                     "bits_ms": dist_case(m, _vp.DIST_L2, _vp.DEPTH_32F, out32, True)})
    for label, metric, depth, out in (("DIST_L1", _vp.DIST_L1, _vp.DEPTH_32F, out32), ("DIST_C", _vp.DIST_C, _vp.DEPTH_32F, out32),
                                      ("DIST_L1 CV_8U", _vp.DIST_L1, _vp.DEPTH_8U, out8)):
        rows.append({"case": label, "mask": masks[0][0], "bits_ms": dist_case(s1, metric, depth, out, True)})
    dist = feature.distance_transform(s1)
    rows.append({"case": "minMaxLoc uint8", "ms": median_ms(lambda: feature.min_max_loc(s1))})
    rows.append({"case": "minMaxLoc float32", "ms": median_ms(lambda: feature.min_max_loc(dist))})
    rows.append({"case": "minMaxLoc float32, mask as bit plane", "ms": median_ms(lambda: feature.min_max_loc(dist, s1))})
    rows.append({"case": "largest_inscribed_circle", "result": repr(feature.largest_inscribed_circle(s1)),
                 "ms": median_ms(lambda: feature.largest_inscribed_circle(s1))})
    tall = np.full((2304, W), 255, np.uint8)
    tall[rng.random(tall.shape) < 0.0001] = 0
    tall_out = DeviceMat(ctx, tall.shape, np.float32)
    for rows_used in (2304, 2048):
        m = mask_of(np.ascontiguousarray(tall[:rows_used]))
        view = tall_out if rows_used == 2304 else DeviceMat(ctx, (rows_used, W), np.float32)
        rows.append({"case": "DIST_L2, column pass %s" % ("from device memory" if rows_used == 2304 else "from LDS strips"), "shape": [rows_used, W],
                     "bits_ms": dist_case(m, _vp.DIST_L2, _vp.DEPTH_32F, view, True)})
    second = yard()
    print(json.dumps({"image": [H, W], "iters": args.iters, "regions": args.regions, "yardsticks_first": first, "yardsticks_second": second, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
