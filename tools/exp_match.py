"""Times template matching (vp_match_template_dev) on one 1080p device image, grey and BGR.

    python tools/exp_match.py [--iters N] [--regions R]

One process, one GPU.  Every figure is the median over R regions of N back-to-back calls, each region bracketed by HIP events on the
context's stream.  One JSON line.  Templates 8^2, 16^2, 32^2, 64^2 and 128^2, cut from the image.  TM_CCORR reads no window sums, so it
is the template kernel and the correlation alone; TM_CCOEFF_NORMED is the whole operator (all integrals and the longest epilogue).
Next to each TM_CCORR time: the rate of useful v_dot4_u32_u8 (results x template bytes / 4 per call) as a fraction of the lane peak,
256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz.  The window sums have no entry of their own: their time is given as TM_SQDIFF (one integral,
S2) minus TM_CCORR at 8^2 and at 128^2 - the integrals cover the whole image, so it should not grow with the template.  best_match end
to end (the map, the search, 32 bytes back, the Python layer).  Yardsticks in the same run, before and after the cases: the 3x3
one-pass GaussianBlur, vp_integral_dev and minMaxLoc on a float32 map of the image's size."""
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
from vision.devmat import DeviceMat  # noqa: E402
from vision.utils import feature  # noqa: E402

ctx = _vp.default_context()
lib = _vp.lib()
W, H = 1920, 1080
LANE_PEAK = 256 * 4 * 32 * 2.4e9          # v_dot4_u32_u8 per second, every lane of every SIMD issuing one each cycle


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


def match_case(img, cn, templ, method, out):
    th, tw = templ.shape[:2]

    def fn():
        _vp.check(lib.vp_match_template_dev(ctx.handle, img.dev_ptr, W * cn, W, H, cn, templ.dev_ptr, tw * cn, tw, th, method, out.dev_ptr, (W - tw + 1) * 4), ctx.handle)
    return median_ms(fn)


def main():
    rng = np.random.default_rng(11)
    host = {1: rng.integers(0, 256, (H, W), dtype=np.uint8), 3: rng.integers(0, 256, (H, W, 3), dtype=np.uint8)}
    dev = {cn: DeviceMat.from_host(ctx, a) for cn, a in host.items()}
    out = DeviceMat(ctx, (H, W), np.float32)
    blurred = DeviceMat(ctx, (H, W), np.uint8)
    integral = DeviceMat(ctx, (H + 1, W + 1), np.int32)
    fmap = DeviceMat.from_host(ctx, rng.random((H, W), dtype=np.float32))

    def yard():
        def gauss():
            _vp.check(lib.vp_gaussian_blur_dev(ctx.handle, dev[1].dev_ptr, W, W, H, 1, 3, 3, 0.0, 0.0, blurred.dev_ptr), ctx.handle)

        def integ():
            _vp.check(lib.vp_integral_dev(ctx.handle, dev[1].dev_ptr, W, W, H, 1, integral.dev_ptr), ctx.handle)
        return {"gaussian_3x3_ms": median_ms(gauss)[0], "integral_ms": median_ms(integ)[0], "min_max_loc_f32_ms": median_ms(lambda: feature.min_max_loc(fmap))[0]}

    first = yard()
    rows = []
    for cn in (1, 3):
        for side in (8, 16, 32, 64, 128):
            t = host[cn][300:300 + side, 700:700 + side].copy()
            templ = DeviceMat.from_host(ctx, t)
            ccorr, spread = match_case(dev[cn], cn, templ, _vp.TM_CCORR, out)
            dots = (W - side + 1) * (H - side + 1) * side * side * cn / 4.0
            row = {"cn": cn, "template": side, "ccorr_ms": ccorr, "ccorr_spread_ms": spread, "udot4_of_lane_peak": round(dots / (ccorr * 1e-3) / LANE_PEAK, 4),
                   "ccoeff_normed_ms": match_case(dev[cn], cn, templ, _vp.TM_CCOEFF_NORMED, out)[0]}
            if side in (8, 128):
                sq, sq_spread = match_case(dev[cn], cn, templ, _vp.TM_SQDIFF, out)
                row.update(sqdiff_ms=sq, sqdiff_spread_ms=sq_spread, window_sums_s2_ms=round(sq - ccorr, 5))
            if side == 32:
                found = feature.best_match(dev[cn], templ)
                assert found[0] == (700, 300), found
                row["best_match_ms"] = median_ms(lambda: feature.best_match(dev[cn], templ))[0]
            rows.append(row)
    second = yard()
    print(json.dumps({"image": [H, W], "iters": args.iters, "regions": args.regions, "yardsticks_first": first, "yardsticks_second": second, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
