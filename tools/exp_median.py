"""Times the median filter (vp_median_blur_dev) on 1080p device images.

    python tools/exp_median.py [--part sizes|window|mask|noise|all] [--iters N] [--regions R]

One process, one GPU.  Every figure is the median over R regions of N back-to-back calls, each region bracketed by HIP events on the
context's stream.  Where two forms are compared they run in the same process, each visited twice, interleaved (a b a b): drift shows as
a gap between the two visits of one form.  One JSON line per part.

  sizes  ms per call for ksize 3, 5, 7, 15, 31, 63 at cn 1 and 3 (default dispatch), and the achieved bytes per second of the ksize 3
         grey case (2 B/px algorithmic: one byte read, one written) as a fraction of the 8 TB/s peak.
  window the same filter on a column window of a wider buffer that starts at an odd address, against the packed image.
  mask   a 10 % speckle mask: the mask kernel (VP_OPT_MEDIAN_MASK 1, with the source's bit plane and from its bytes) against the general
         kernels (0) at ksize 3, 5 (networks) and 7, 15 (histograms).
  noise  speckle straight into the labelling: grey noise >= lo at 2 / 10 / 50 % density -> connected_components, alone and with a
         median_blur(3) in front, per frame (the filter has no batched entry)."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--part", default="all")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--regions", type=int, default=7)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cuauv-vision-pipeline_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (shares the HIP runtime with libvp)

import frames as F  # noqa: E402
from vision import _vp  # noqa: E402
from vision.devmat import DeviceMat, _DevBuf  # noqa: E402
from vision.utils import color, feature, transform  # noqa: E402

ctx = _vp.default_context()
lib = _vp.lib()
W, H = 1920, 1080
PEAK_BPS = 8e12


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
    return round(statistics.median(t), 5)


def call(src, dst, cn, k, hint=0, plane=None, out_plane=None):
    def fn():
        _vp.check(lib.vp_median_blur_dev(ctx.handle, src.dev_ptr, W * cn, W, H, cn, k, hint, None if plane is None else plane.ptr, dst.dev_ptr,
                                         None if out_plane is None else out_plane.ptr, None), ctx.handle)
    return fn


def interleaved(forms):
    """forms: name -> (setup, fn); every form timed twice, a b a b"""
    t = {}
    for _ in range(2):
        for name, (setup, fn) in forms.items():
            setup()
            t.setdefault(name, []).append(median_ms(fn))
    return t


def part_sizes():
    bgr = F.s1_buoy(0, W, H)
    rows = []
    for cn in (1, 3):
        img = np.ascontiguousarray(bgr[:, :, 1]) if cn == 1 else bgr
        src, dst = DeviceMat.from_host(ctx, img), DeviceMat(ctx, img.shape)
        for k in (3, 5, 7, 15, 31, 63):
            rows.append({"cn": cn, "k": k, "ms": median_ms(call(src, dst, cn, k), iters=args.iters if k <= 15 else max(2, args.iters // 5))})
    ms3 = next(r["ms"] for r in rows if r["cn"] == 1 and r["k"] == 3)
    bps = 2.0 * W * H / (ms3 * 1e-3)
    print(json.dumps({"part": "sizes", "image": [H, W], "iters": args.iters, "regions": args.regions, "rows": rows,
                      "k3_grey_bytes_per_s": round(bps, 0), "k3_grey_fraction_of_8TBps": round(bps / PEAK_BPS, 4)}), flush=True)


def part_window():
    """a column window of a wider buffer whose first byte is not 4-byte aligned (every staged dword of the networks is assembled from
    bytes) against the packed, aligned image of the same pixels"""
    rng = np.random.default_rng(1)
    rows = []
    for cn in (1, 3):
        wide = rng.integers(0, 256, (H, W + 64, cn), dtype=np.uint8)
        buf = DeviceMat.from_host(ctx, wide)
        packed = DeviceMat.from_host(ctx, np.ascontiguousarray(wide[:, 31:31 + W]))
        dst = DeviceMat(ctx, (H, W, cn))
        for k in (3, 5, 15):
            def win():
                _vp.check(lib.vp_median_blur_dev(ctx.handle, buf.dev_ptr + 31 * cn, (W + 64) * cn, W, H, cn, k, 0, None, dst.dev_ptr, None, None), ctx.handle)
            rows.append(dict({"cn": cn, "k": k}, **interleaved({"packed_ms": (lambda: None, call(packed, dst, cn, k)), "window_ms": (lambda: None, win)})))
    print(json.dumps({"part": "window", "image": [H, W], "rows": rows}), flush=True)


def part_mask():
    rng = np.random.default_rng(0)
    gray = np.where(rng.random((H, W)) < 0.10, 200, 10).astype(np.uint8)
    mask = color.range_threshold(DeviceMat.from_host(ctx, gray), 150, 255)
    plane = mask.bit_plane(ctx)
    assert plane is not None
    dst, out_plane = DeviceMat(ctx, (H, W)), _DevBuf(ctx, H * (W // 64) * 8)
    rows = []
    try:
        for k in (3, 5, 7, 15):
            forms = {"general_ms": (lambda: ctx.set_option(_vp.OPT_MEDIAN_MASK, 0), call(mask, dst, 1, k, 1)),
                     "mask_from_plane_ms": (lambda: ctx.set_option(_vp.OPT_MEDIAN_MASK, 1), call(mask, dst, 1, k, 1, plane, out_plane)),
                     "mask_from_bytes_ms": (lambda: ctx.set_option(_vp.OPT_MEDIAN_MASK, 1), call(mask, dst, 1, k, 1, None, out_plane))}
            rows.append(dict({"k": k, "general_kernel": "network" if k <= 5 else "histogram"}, **interleaved(forms)))
    finally:
        ctx.set_option(_vp.OPT_MEDIAN_MASK, -1)
    print(json.dumps({"part": "mask", "image": [H, W], "speckle": 0.10, "rows": rows}), flush=True)


def part_noise():
    rows = []
    gray = np.ascontiguousarray(F.s3_noise(0, W, H)[:, :, 1])
    for pct in (2, 10, 50):
        lo = int(np.percentile(gray, 100 - pct))
        g = DeviceMat.from_host(ctx, gray)
        dens = float((gray >= lo).mean())

        def label_alone():
            feature.connected_components(color.range_threshold(g, lo, 255), max_labels=65536, want_labels=True)

        def filter_then_label():
            feature.connected_components(transform.median_blur(color.range_threshold(g, lo, 255), 3), max_labels=65536, want_labels=True)

        def filter_alone():
            transform.median_blur(color.range_threshold(g, lo, 255), 3)
        t = interleaved({"label_ms": (lambda: None, label_alone), "filter_label_ms": (lambda: None, filter_then_label),
                         "threshold_filter_ms": (lambda: None, filter_alone)})
        n0 = feature.connected_components(color.range_threshold(g, lo, 255), max_labels=65536, want_labels=False)[0]
        n1 = feature.connected_components(transform.median_blur(color.range_threshold(g, lo, 255), 3), max_labels=65536, want_labels=False)[0]
        rows.append(dict({"noise_pct": pct, "density": round(dens, 4), "labels_raw": int(n0), "labels_filtered": int(n1)}, **t))
    print(json.dumps({"part": "noise", "image": [H, W], "per": "frame", "rows": rows}), flush=True)


if __name__ == "__main__":
    for name, fn in (("sizes", part_sizes), ("window", part_window), ("mask", part_mask), ("noise", part_noise)):
        if args.part in (name, "all"):
            fn()
