"""Times the moment kernels (vp_moments_dev, vp_label_moments_dev) on one 1080p device image.

    python tools/exp_moments.py [--iters N] [--regions R]

One process, one GPU.  Every figure is the median over R regions of N back-to-back calls, each region bracketed by HIP events on the
context's stream; every call reads the image once, copies its small table back and synchronises.  One JSON line.  Cases: the grey
image, the S1 byte mask (binary), the same mask through its bit plane; the label moments of the S1 mask's labels and of 2 % and 10 %
speckle, with the table (above 768 labels: its first 64 rows) in each block's LDS and all of it in device memory
(VP_OPT_LABEL_MOMENTS_LDS 1 / 0), for table sizes on both sides of what LDS holds.  Yardsticks, timed in the same run before and after
the cases: vp_count_nonzero_u8_dev and vp_hist_u8_dev on the same image - both read it once and synchronise."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=30)
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


def main():
    bgr = F.s1_buoy(0, W, H)
    grey = DeviceMat.from_host(ctx, np.ascontiguousarray(bgr[:, :, 1]))
    mask = cv.inRange(cv.cvtColor(DeviceMat.from_host(ctx, bgr), cv.COLOR_BGR2LAB), (0, 150, 0), (255, 255, 255))
    bits = mask.bit_plane(ctx)
    out = np.zeros(10, np.uint64)
    hist = np.zeros(256, np.uint32)
    count = _vp.C.c_uint64(0)

    def yard():
        def nz():
            _vp.check(lib.vp_count_nonzero_u8_dev(ctx.handle, grey.dev_ptr, W * H, _vp.C.byref(count)), ctx.handle)

        def hi():
            _vp.check(lib.vp_hist_u8_dev(ctx.handle, grey.dev_ptr, W * H, hist.ctypes.data), ctx.handle)
        return {"count_nonzero_ms": median_ms(nz), "hist_ms": median_ms(hi)}

    first = yard()
    rows = []

    def raster(name, src, binary, bp):
        def fn():
            _vp.check(lib.vp_moments_dev(ctx.handle, src.dev_ptr, W, W, H, binary, bp, out.ctypes.data), ctx.handle)
        rows.append({"case": name, "ms": median_ms(fn)})

    raster("grey", grey, 0, None)
    raster("byte mask, binary", mask, 1, None)
    if bits is not None:
        raster("bit plane", mask, 1, bits.ptr)

    rng = np.random.default_rng(7)
    sources = [("S1 mask", mask)]
    for pct in (2, 10):
        sources.append((f"{pct} % speckle", DeviceMat.from_host(ctx, ((rng.random((H, W)) < pct / 100) * 255).astype(np.uint8))))
    for name, m in sources:
        n, labels, _, _ = feature.connected_components(m, max_labels=1 << 20)
        for nl in sorted({n, 64, 256, 768, 769, 4096}):
            if nl < n:
                continue                                    # every label has its row: the kernel adds for all of them
            table = np.zeros((nl, 10), np.uint64)

            def fn():
                _vp.check(lib.vp_label_moments_dev(ctx.handle, labels.dev_ptr, 4 * W, W, H, nl, table.ctypes.data), ctx.handle)
            r = {"case": "labels of " + name, "components": n, "nlabels": nl}
            for key, opt in (("lds_ms", 1), ("global_ms", 0)):
                ctx.set_option(_vp.OPT_LABEL_MOMENTS_LDS, opt)
                r[key] = median_ms(fn)
            ctx.set_option(_vp.OPT_LABEL_MOMENTS_LDS, -1)
            rows.append(r)
    second = yard()
    print(json.dumps({"image": [H, W], "iters": args.iters, "regions": args.regions, "yardsticks_first": first, "yardsticks_second": second, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
