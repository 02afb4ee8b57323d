"""Times Lab -> BGR and the two white balances on one 1080p frame in HBM (device entry points, nothing copied per call).

    python tools/exp_white_balance.py [--iters N]

Prints one JSON line: milliseconds per image (HIP events around N back-to-back calls) for lab_to_bgr (interleaved output only),
white_balance_bgr and white_balance_bgr_blur at k = 5 and k = 255.  Run it under `rocprofv3 --kernel-trace --stats` for the
per-kernel split."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cuauv-vision-pipeline_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (shares the HIP runtime with libvp)

import frames as F  # noqa: E402
from vision import _vp  # noqa: E402
from vision.devmat import DeviceMat  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    ctx = _vp.default_context()
    lib = _vp.lib()
    img = F.s1_buoy(0, 1920, 1080)
    h, w = img.shape[:2]
    src = DeviceMat.from_host(ctx, img)
    dst = DeviceMat(ctx, (h, w, 3))

    def lab2bgr():
        _vp.check(lib.vp_cvt_color_dev(ctx.handle, _vp.LAB2BGR, src.dev_ptr, w * 3, w, h, dst.dev_ptr, None), ctx.handle)

    def wb(k):
        return lambda: _vp.check(lib.vp_white_balance_dev(ctx.handle, src.dev_ptr, w * 3, w, h, k, dst.dev_ptr, None), ctx.handle)

    out = {"image": [h, w], "iters": args.iters}
    for name, fn in (("lab_to_bgr", lab2bgr), ("white_balance_bgr", wb(_vp.WB_GLOBAL_MEAN)), ("white_balance_bgr_blur_k5", wb(5)),
                     ("white_balance_bgr_blur_k255", wb(255))):
        for _ in range(10):
            fn()
        ctx.synchronize()
        ctx.timer_start()
        for _ in range(args.iters):
            fn()
        out[name + "_ms"] = round(ctx.timer_stop() / args.iters, 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
