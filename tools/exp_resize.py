"""Times cv2.resize (INTER_LINEAR, 8-bit) of one 1080p BGR frame to 1366x768 and the detector's letterbox of the same frame to 640x640.

    python tools/exp_resize.py [--iters N]

Prints one JSON line: milliseconds per call of the letterbox's device entry (frame already in HBM, HIP events around N back-to-back
calls) and of the resize's host entry (for scale only: it includes both copies).  Run it under `rocprofv3 --kernel-trace --stats` for
the kernel times of k_resize_u8 and k_letterbox."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cuauv-vision-pipeline_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402  (shares the HIP runtime with libvp)

import frames as F  # noqa: E402
from vision import _vp  # noqa: E402
from vision.devmat import DeviceMat  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    ctx = _vp.default_context()
    lib = _vp.lib()
    img = F.s1_buoy(0, 1920, 1080)
    h, w = img.shape[:2]
    src = DeviceMat.from_host(ctx, img)
    lb = torch.empty((3, 640, 640), dtype=torch.float32, device=torch.device("cuda", ctx.device))
    out = {"image": [h, w], "iters": args.iters}

    def letterbox():
        _vp.check(lib.vp_letterbox_dev(ctx.handle, src.dev_ptr, w, h, 640, 640, 114, lb.data_ptr(), None), ctx.handle)
    res = np.empty((768, 1366, 3), np.uint8)

    def resize():
        _vp.check(lib.vp_resize_u8(ctx.handle, _vp.ptr(img), w, h, 3, 1366, 768, _vp.ptr(res)), ctx.handle)
    for name, fn in (("letterbox_640_dev_ms", letterbox), ("resize_1366x768_host_ms", resize)):
        for _ in range(3):
            fn()
        ctx.synchronize()
        ctx.timer_start()
        for _ in range(args.iters):
            fn()
        out[name] = round(ctx.timer_stop() / args.iters, 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
