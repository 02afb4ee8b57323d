"""Times stereo rectification and reprojection (vp_rectify_pair_dev, vp_reproject_to_3d_dev) on one 1280 x 720 BGR pair, the reference's
HD720, beside the same work composed from the existing entries.

    python tools/exp_rectify.py [--iters N] [--regions R]

One process, one GPU.  Every figure is the median over R regions of N back-to-back calls, each region bracketed by HIP events on the
context's stream and ended by a synchronise: whole calls, launches included.  Rows: vp_rectify_pair_dev with grey results only and with
both colour results; the composition, two vp_remap_fixed_dev and two vp_cvt_color_dev (four launches, two colour intermediates);
vp_reproject_to_3d_dev on an int16 disparity image; StereoRig.planes from a raw side-by-side frame for both matchers (the Python layer
on DeviceMats, nothing leaving HBM).  Beside each rectify time stand the bytes the row must move, computed from the shapes (6 bytes of
table, cn of source and 1 of grey per output pixel and eye, + cn where colour is kept; the composition writes and reads the colour
image once more and reads the table's 6 bytes), and the rate that makes.  Yardsticks in the same run: RemapTable.apply on one BGR eye
and the 3 x 3 one-pass GaussianBlur.  The fused results are compared with the composition's.  One table, then one JSON line."""
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "cuauv-vision-pipeline_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (shares the HIP runtime with libvp)

from vision import _vp  # noqa: E402
from vision.devmat import DeviceMat  # noqa: E402
from vision.utils import stereo  # noqa: E402

ctx = _vp.default_context()
lib = _vp.lib()
W, H, CN = 1280, 720, 3


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
    return round(statistics.median(t), 5), round(max(t) - min(t), 5)


def raw_frame():
    """a textured side-by-side BGR frame, the right eye 40 pixels over"""
    rng = np.random.default_rng(21)
    a = rng.integers(0, 256, (H + 2, W + 40 + 2, CN)).astype(np.int32)
    base = (sum(a[i:i + H, j:j + W + 40] for i in range(3) for j in range(3)) // 9).astype(np.uint8)
    return np.ascontiguousarray(np.concatenate([base[:, :W], base[:, 40:40 + W]], axis=1))


def main():
    K1 = np.array([[700.0, 0, 642.0], [0, 701.0, 358.0], [0, 0, 1]])
    K2 = np.array([[698.0, 0, 637.0], [0, 699.5, 362.0], [0, 0, 1]])
    rig = stereo.StereoRig(K1, [-0.17, 0.026, 0.0004, -0.0003, -0.001], K2, [-0.168, 0.025, -0.0002, 0.0005, -0.001], (W, H), stereo.rodrigues([0.004, -0.009, 0.006]),
                           [-0.12, 0.001, -0.0008])
    frame = DeviceMat.from_host(ctx, raw_frame())
    lp, rp, stride = frame.dev_ptr, frame.dev_ptr + W * CN, 2 * W * CN
    tl, tr = rig.tables
    grey = [DeviceMat(ctx, (H, W), np.uint8) for _ in range(2)]
    col = [DeviceMat(ctx, (H, W, CN), np.uint8) for _ in range(2)]
    grey2 = [DeviceMat(ctx, (H, W), np.uint8) for _ in range(2)]
    col2 = [DeviceMat(ctx, (H, W, CN), np.uint8) for _ in range(2)]
    zero = np.zeros(4, np.uint8)

    def fused(colour):
        _vp.check(lib.vp_rectify_pair_dev(ctx.handle, lp, stride, rp, stride, W, H, CN, tl.xy.dev_ptr, tl.frac.dev_ptr, tr.xy.dev_ptr, tr.frac.dev_ptr, W, H,
                                          grey[0].dev_ptr, W, grey[1].dev_ptr, W, col[0].dev_ptr if colour else None, W * CN, col[1].dev_ptr if colour else None, W * CN),
                  ctx.handle)

    def composed():
        for e, (p, t) in enumerate(((lp, tl), (rp, tr))):
            _vp.check(lib.vp_remap_fixed_dev(ctx.handle, p, stride, W, H, CN, t.xy.dev_ptr, t.frac.dev_ptr, W, H, _vp.INTER_LINEAR, _vp.BORDER_CONSTANT, zero.ctypes.data,
                                             col2[e].dev_ptr), ctx.handle)
            _vp.check(lib.vp_cvt_color_dev(ctx.handle, _vp.BGR2GRAY, col2[e].dev_ptr, W * CN, W, H, grey2[e].dev_ptr, None), ctx.handle)

    px = 2 * W * H
    rows = []
    # alternate the three forms so that a drift of the box shows in all of them
    t = {"fused_grey": [], "fused_colour": [], "composed": []}
    for _ in range(3):
        t["fused_grey"].append(median_ms(lambda: fused(False)))
        t["composed"].append(median_ms(composed))
        t["fused_colour"].append(median_ms(lambda: fused(True)))
    moved = {"fused_grey": px * (6 + CN + 1), "fused_colour": px * (6 + CN + 1 + CN), "composed": px * (6 + CN + CN + CN + 1)}
    for k in ("fused_grey", "fused_colour", "composed"):
        ms = statistics.median(m for m, _ in t[k])
        rows.append({"row": k, "ms": ms, "rounds_ms": [m for m, _ in t[k]], "spread_ms": max(s for _, s in t[k]), "mb": round(moved[k] / 1e6, 1),
                     "gb_per_s": round(moved[k] / (ms * 1e-3) / 1e9, 1)})
    fused(True)
    composed()
    same = all(np.array_equal(a.host_copy(), b.host_copy()) for a, b in zip(grey + col, grey2 + col2))

    disp = rig.disparity(frame, num_disparities=64)
    xyz = DeviceMat(ctx, (H, W, 3), np.float32)
    q = np.ascontiguousarray(rig.Q)

    def reproject():
        _vp.check(lib.vp_reproject_to_3d_dev(ctx.handle, disp.dev_ptr, 2 * W, 0, W, H, q.ctypes.data, -16, xyz.dev_ptr, 12 * W), ctx.handle)
    ms, spread = median_ms(reproject)
    rows.append({"row": "reproject_i16", "ms": ms, "spread_ms": spread, "mb": round(W * H * 14 / 1e6, 1), "gb_per_s": round(W * H * 14 / (ms * 1e-3) / 1e9, 1)})
    for matcher in ("bm", "sgm"):
        ms, spread = median_ms(lambda: rig.planes(frame, matcher=matcher, num_disparities=64))
        rows.append({"row": f"rig_planes_{matcher}_n64", "ms": ms, "spread_ms": spread})
    left = DeviceMat.from_host(ctx, np.ascontiguousarray(frame.host_copy()[:, :W]))
    blurred = DeviceMat(ctx, (H, W), np.uint8)

    def gauss():
        _vp.check(lib.vp_gaussian_blur_dev(ctx.handle, grey[0].dev_ptr, W, W, H, 1, 3, 3, 0.0, 0.0, blurred.dev_ptr), ctx.handle)
    yard = {"remap_table_apply_bgr_ms": median_ms(lambda: tl.apply(left))[0], "gaussian_3x3_ms": median_ms(gauss)[0]}
    print("%-24s %10s %10s %8s %10s" % ("row", "ms", "spread", "MB", "GB/s"))
    for r in rows:
        print("%-24s %10.4f %10.4f %8s %10s" % (r["row"], r["ms"], r["spread_ms"], r.get("mb", ""), r.get("gb_per_s", "")))
    for k, v in yard.items():
        print("%-40s %10.4f" % (k, v))
    print("fused == composed:", same)
    print(json.dumps({"image": [H, W, CN], "iters": args.iters, "regions": args.regions, "fused_equals_composed": bool(same), "yardsticks": yard, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
