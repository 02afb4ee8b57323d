"""Times the Gaussian adaptive threshold on one 1080p grey frame in HBM (device entry point, nothing copied per call).

    python tools/exp_adaptive.py [--iters N]

Prints one JSON line: milliseconds per image (HIP events around N back-to-back calls) at block sizes 11, 31, 151 and 511, with the
mean method's time at 11 and 31 beside them (host entry, for scale only: it includes the copies).  Run it under
`rocprofv3 --kernel-trace --stats` for the split between k_agauss_h and k_agauss_v."""
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
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    ctx = _vp.default_context()
    lib = _vp.lib()
    img = np.ascontiguousarray(F.s1_buoy(0, 1920, 1080)[:, :, 1])
    h, w = img.shape
    src = DeviceMat.from_host(ctx, img)
    dst = DeviceMat(ctx, (h, w))
    out = {"image": [h, w], "iters": args.iters}
    for block in (11, 31, 151, 511):
        def fn():
            _vp.check(lib.vp_adaptive_threshold_gaussian_dev(ctx.handle, src.dev_ptr, w, w, h, 255.0, 0, block, 2.0, dst.dev_ptr), ctx.handle)
        for _ in range(3):
            fn()
        ctx.synchronize()
        ctx.timer_start()
        for _ in range(args.iters):
            fn()
        out[f"gaussian_b{block}_ms"] = round(ctx.timer_stop() / args.iters, 5)
    res = np.empty_like(img)
    for block in (11, 31):
        def mean():
            _vp.check(lib.vp_adaptive_threshold_mean_u8(ctx.handle, _vp.ptr(img), w, h, 255.0, 0, block, 2.0, _vp.ptr(res)), ctx.handle)
        mean()
        ctx.synchronize()
        ctx.timer_start()
        for _ in range(args.iters):
            mean()
        out[f"mean_host_b{block}_ms"] = round(ctx.timer_stop() / args.iters, 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
