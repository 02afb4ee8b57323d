"""Times the speckle filter (vp_filter_speckles_dev), the surface normals (vp_normals_from_depth_dev) and the chain `stereo_planes` on
1280 x 720 device images, the reference's HD720.

    python tools/exp_speckle.py [--iters N] [--regions R]

One process, one GPU.  Every device figure is the median over R regions of N back-to-back calls, each region bracketed by HIP events on
the context's stream and ended by a synchronise: whole calls, launches included.  Rows of `filter_speckles` (max_speckle_size 100,
max_diff 32): the `disparity` (64 / 15) of this tool's synthetic pair (one scene at disparity 40 under noise in the right image, so
that the matcher leaves islands); an all-valid constant image (one region: the counting hot spot); a constant image with 2 % and with
10 % of its pixels set to a far value at random (speckle); a one-pixel serpentine that crosses every tile edge.  Every result is
compared with vp_filter_speckles_host's once, and the host routine is timed on one core (one call each, host clock).  Then
`normals_from_depth`, and `stereo_planes` end to end against `stereo_depth`.  Yardsticks in the same run: `disparity` at 64 / 15,
vp_ccl_bits_dev of a mask of the same size, and the 3 x 3 one-pass GaussianBlur.  One table, then one JSON line."""
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
NEW_VAL, SIZE, DIFF = -16, 100, 32


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
    right = np.clip(base[:, 40:40 + W].astype(np.int32) + rng.integers(-60, 61, (H, W)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(base[:, :W]), np.ascontiguousarray(right)


def speckled(share, seed):
    img = np.full((H, W), 640, np.int16)
    img[np.random.default_rng(seed).random((H, W)) < share] = 2000
    return img


def serpentine():
    img = np.full((H, W), NEW_VAL, np.int16)
    rows = range(0, H - 1, 2)
    for k, y in enumerate(rows):
        img[y, :] = 640
        if y + 2 in rows:
            img[y + 1, W - 1 if k % 2 == 0 else 0] = 640
    return img


def main():
    left, right = pair()
    dl, dr = DeviceMat.from_host(ctx, left), DeviceMat.from_host(ctx, right)
    tile = (C.c_int32 * 5)()
    ws = C.c_size_t()
    _vp.check(lib.vp_filter_speckles_plan(W, H, C.byref(ws), tile))

    blurred = DeviceMat(ctx, (H, W), np.uint8)
    disp_dev = DeviceMat(ctx, (H, W), np.int16)
    mask = np.zeros((H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for cy, cx, r in ((200, 300, 90), (500, 900, 140), (360, 640, 40)):
        mask[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = 1
    bits = DeviceMat.from_host(ctx, np.packbits(mask, axis=1, bitorder="little").view(np.uint64))
    labels = DeviceMat(ctx, (H, W), np.int32)
    stats, cents, nlab = np.zeros((64, 5), np.int32), np.zeros((64, 2), np.float64), C.c_int32()

    def gauss():
        _vp.check(lib.vp_gaussian_blur_dev(ctx.handle, dl.dev_ptr, W, W, H, 1, 3, 3, 0.0, 0.0, blurred.dev_ptr), ctx.handle)

    def bm():
        _vp.check(lib.vp_stereo_bm_dev(ctx.handle, dl.dev_ptr, W, dr.dev_ptr, W, W, H, 64, 15, 0, 31, 10, 15, disp_dev.dev_ptr, 2 * W), ctx.handle)

    def ccl():
        _vp.check(lib.vp_ccl_bits_dev(ctx.handle, bits.dev_ptr, W, H, _vp.CCL_PIXEL, labels.dev_ptr, stats.ctypes.data,
                                      cents.ctypes.data, 64, C.byref(nlab)), ctx.handle)

    yard = {"gaussian_3x3_ms": median_ms(gauss)[0], "disparity_n64_b15_ms": median_ms(bm)[0], "ccl_bits_dev_ms": median_ms(ccl)[0], "ccl_labels": int(nlab.value)}
    bm()
    images = [("disparity of the pair", disp_dev.host_copy()), ("constant, one region", np.full((H, W), 640, np.int16)), ("2 % speckle", speckled(0.02, 1)),
              ("10 % speckle", speckled(0.10, 2)), ("serpentine", serpentine())]
    rows = []
    out = DeviceMat(ctx, (H, W), np.int16)
    for name, img in images:
        src = DeviceMat.from_host(ctx, img)

        def run():
            _vp.check(lib.vp_filter_speckles_dev(ctx.handle, src.dev_ptr, 2 * W, W, H, NEW_VAL, SIZE, DIFF, out.dev_ptr, 2 * W), ctx.handle)
        ms, spread = median_ms(run)
        got = out.host_copy()
        want = np.empty((H, W), np.int16)
        t0 = time.perf_counter()
        _vp.check(lib.vp_filter_speckles_host(img.ctypes.data, 2 * W, W, H, NEW_VAL, SIZE, DIFF, want.ctypes.data, 2 * W))
        host_ms = (time.perf_counter() - t0) * 1e3
        rows.append({"image": name, "filter_speckles_dev_ms": ms, "spread_ms": spread, "host_one_core_ms": round(host_ms, 1), "removed": int((got != img).sum()),
                     "equals_host": bool(np.array_equal(got, want))})
    depth = stereo.stereo_depth(dl, dr, FOCAL, BASELINE)
    extra = {"normals_from_depth_ms": median_ms(lambda: stereo.normals_from_depth(depth, FOCAL))[0],
             "normals_encoded_guarded_ms": median_ms(lambda: stereo.normals_from_depth(depth, FOCAL, max_jump_m=0.5, encode=True))[0],
             "stereo_depth_ms": median_ms(lambda: stereo.stereo_depth(dl, dr, FOCAL, BASELINE))[0],
             "stereo_planes_ms": median_ms(lambda: stereo.stereo_planes(dl, dr, FOCAL, BASELINE))[0],
             "stereo_planes_no_filter_ms": median_ms(lambda: stereo.stereo_planes(dl, dr, FOCAL, BASELINE, speckle_window_size=0))[0]}
    yard["gaussian_3x3_after_ms"] = median_ms(gauss)[0]
    print("tile %d x %d, grid %d x %d, workspace %d bytes" % (tile[0], tile[1], tile[2], tile[3], ws.value))
    print("%-24s %12s %8s %14s %9s %6s" % ("image", "filter ms", "spread", "host 1 core ms", "removed", "equal"))
    for r in rows:
        print("%-24s %12.4f %8.4f %14.1f %9d %6s" % (r["image"], r["filter_speckles_dev_ms"], r["spread_ms"], r["host_one_core_ms"], r["removed"], r["equals_host"]))
    for k, v in {**extra, **yard}.items():
        print("%-40s %10.4f" % (k, v))
    print(json.dumps({"image": [H, W], "iters": args.iters, "regions": args.regions, "tile": [tile[0], tile[1]], "yardsticks": yard, "rows": rows, **extra}), flush=True)


if __name__ == "__main__":
    main()
