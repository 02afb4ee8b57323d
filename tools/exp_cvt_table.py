"""Time per 1080p conversion of every colour code added beside the first eight, on device images (vp_cvt_color_dev, interleaved result
only), next to VP_BGR2YCRCB and the other BGR-order siblings timed in the same run.  HIP events around a warmed-up loop of `calls`
launches give one sample (device microseconds per call); every code is sampled `rounds` times, the codes taken in turn within a round so
that drift of the box lands on all of them; the table holds the median and the smallest and largest sample.
usage: python tools/exp_cvt_table.py [calls] [rounds]        (json on the last line)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "cuauv-vision-pipeline_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import frames as F
from vision import _vp
from vision.devmat import DeviceMat

SIBLINGS = ["BGR2YCRCB", "BGR2GRAY", "BGR2HSV", "BGR2HLS", "BGR2LAB", "LAB2BGR", "HSV2BGR", "GRAY2BGR"]
NEW = ["BGR2YUV", "YUV2BGR", "YCRCB2BGR", "BGR2XYZ", "XYZ2BGR", "HLS2BGR", "BGR2RGB", "RGB2GRAY", "RGB2HSV", "HSV2RGB", "RGB2HLS", "HLS2RGB",
       "RGB2LAB", "LAB2RGB", "RGB2YCRCB", "YCRCB2RGB", "RGB2YUV", "YUV2RGB", "RGB2XYZ", "XYZ2RGB", "BGRA2BGR", "RGBA2BGR", "BGR2BGRA",
       "BGR2RGBA", "BGRA2RGBA", "GRAY2BGRA", "BGRA2GRAY", "RGBA2GRAY"]


def measure(calls=200, rounds=7):
    ctx = _vp.default_context()
    lib = _vp.lib()
    frame = F.s1_buoy(0)
    h, w = frame.shape[:2]
    rng = np.random.default_rng(0)
    src = {3: DeviceMat.from_host(ctx, frame), 1: DeviceMat.from_host(ctx, np.ascontiguousarray(frame[:, :, 1])),
           4: DeviceMat.from_host(ctx, np.dstack([frame, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)]))}
    dst = DeviceMat(ctx, (h, w, 4))
    runs = {}
    for name in SIBLINGS + NEW:
        code = getattr(_vp, name)
        scn, dcn = _vp.CVT_CHANNELS.get(code, (3, 3))
        s, d = src[scn].dev_ptr, dst.dev_ptr
        runs[name] = (lambda code=code, s=s, d=d, scn=scn: _vp.check(lib.vp_cvt_color_dev(ctx.handle, code, s, w * scn, w, h, d, None), ctx.handle), (scn + dcn) * w * h)
    for fn, _ in runs.values():
        for _ in range(10):
            fn()
    ctx.synchronize()
    samples = {name: [] for name in runs}
    for _ in range(rounds):
        for name, (fn, _) in runs.items():
            ctx.timer_start()
            for _ in range(calls):
                fn()
            samples[name].append(1e3 * ctx.timer_stop() / calls)
    out = {"size": [w, h], "calls": calls, "rounds": rounds, "codes": {}}
    for name, (_, nbytes) in runs.items():
        t = sorted(samples[name])
        med = float(np.median(t))
        out["codes"][name] = {"us_median": round(med, 2), "us_min": round(t[0], 2), "us_max": round(t[-1], 2), "bytes": nbytes,
                              "tb_per_s": round(nbytes / med * 1e-6, 3), "new": name in NEW}
    return out


if __name__ == "__main__":
    r = measure(int(sys.argv[1]) if len(sys.argv) > 1 else 200, int(sys.argv[2]) if len(sys.argv) > 2 else 7)
    for k, v in r["codes"].items():
        print("%-10s %s" % (k, v))
    print(json.dumps(r))
