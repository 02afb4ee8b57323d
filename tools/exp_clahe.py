"""Times cv2.equalizeHist and CLAHE (vp_equalize_hist_dev, vp_clahe_dev, vision.utils.color.clahe_bgr) on one 1080p device image.

    python tools/exp_clahe.py [--iters N] [--regions R]

One process, one GPU.  Every figure is the median over R regions of N back-to-back calls, each region bracketed by HIP events on the
context's stream.  One JSON line.  Per case: ms per call, the achieved bytes per second against the algorithmic bytes (CLAHE reads the
plane twice and writes it once, 3 B/px; equalizeHist the same), and the ratio of that rate to the rate vp_gaussian_blur_dev (3x3, the
one-pass form, 1 read + 1 written) reaches on the same plane in the same run.  The blur is timed before and after the cases; both
visits are reported.  CLAHE runs at grids (4, 4), (8, 8), (16, 16), clip limits 2 and 40, with the planned share of blocks per tile
(VP_OPT_CLAHE_SPLIT 0) and every forced one; clahe_bgr is the whole Lab round trip through the Python operators."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--regions", type=int, default=9)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cuauv-vision-pipeline_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (shares the HIP runtime with libvp)

import frames as F  # noqa: E402
from vision import _vp  # noqa: E402
from vision.devmat import DeviceMat  # noqa: E402
from vision.utils import color  # noqa: E402

ctx = _vp.default_context()
lib = _vp.lib()
W, H = 1920, 1080
SPLITS = [0, 1, 2, 4, 8, 16, 32, 64]


def median_ms(fn, iters=None):
    iters = iters or args.iters
    for _ in range(3):
        fn()
    ctx.synchronize()
    t = []
    for _ in range(args.regions):
        ctx.timer_start()
        for _ in range(iters):
            fn()
        t.append(ctx.timer_stop() / iters)
    return statistics.median(t)


def main():
    bgr = F.s1_buoy(0, W, H)
    dbgr = DeviceMat.from_host(ctx, bgr)
    src = DeviceMat.from_host(ctx, np.ascontiguousarray(bgr[:, :, 1]))
    dst = DeviceMat(ctx, (H, W))
    ctx.set_option(_vp.OPT_BLUR_ONEPASS, 1)

    def blur():
        def fn():
            _vp.check(lib.vp_gaussian_blur_dev(ctx.handle, src.dev_ptr, W, W, H, 1, 3, 3, 0.0, 0.0, dst.dev_ptr), ctx.handle)
        ms = median_ms(fn)
        return ms, 2.0 * W * H / (ms * 1e-3)

    blur_first = blur()
    rows = []

    def row(name, ms, nbytes, **extra):
        r = {"case": name, "ms": round(ms, 5), "bytes": int(nbytes), "bytes_per_s": round(nbytes / (ms * 1e-3), 0)}
        r.update(extra)
        rows.append(r)

    def eq():
        _vp.check(lib.vp_equalize_hist_dev(ctx.handle, src.dev_ptr, W, W, H, dst.dev_ptr), ctx.handle)
    row("equalize_hist", median_ms(eq), 3 * W * H)
    for grid in ((4, 4), (8, 8), (16, 16)):
        for clip in (2.0, 40.0):
            for split in SPLITS:
                ctx.set_option(_vp.OPT_CLAHE_SPLIT, split)

                def fn():
                    _vp.check(lib.vp_clahe_dev(ctx.handle, src.dev_ptr, W, W, H, clip, grid[0], grid[1], dst.dev_ptr), ctx.handle)
                row("clahe", median_ms(fn), 3 * W * H, grid=list(grid), clip=clip, split=split)
    ctx.set_option(_vp.OPT_CLAHE_SPLIT, 0)

    def bgr_fn():
        color.clahe_bgr(dbgr, 2.0, (8, 8))
    row("clahe_bgr", median_ms(bgr_fn, max(1, args.iters // 5)), 3 * W * H * 3)
    blur_second = blur()
    ctx.set_option(_vp.OPT_BLUR_ONEPASS, -1)
    ref = (blur_first[1] + blur_second[1]) / 2
    for r in rows:
        r["rate_vs_blur"] = round(r["bytes_per_s"] / ref, 3)
    print(json.dumps({"image": [H, W], "iters": args.iters, "regions": args.regions,
                      "blur3x3_onepass": {"ms": [round(blur_first[0], 5), round(blur_second[0], 5)],
                                          "bytes_per_s": [round(blur_first[1], 0), round(blur_second[1], 0)]},
                      "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
