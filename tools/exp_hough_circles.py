"""cv2.HoughCircles (HOUGH_GRADIENT) on the GPU (csrc/vp_hough_circles.hip): 1080p frames held on the device, through the C-ABI call,
radius histograms in LDS and in device memory, and the CPU statement of the tests (tests/hough_circles_restate.py, numpy on one core) as
the baseline where it finishes in seconds.  Cases: buoy frame 0 (tests/frames.py s1_buoy, green plane) at the reference's defaults
(param1 = param2 = 100, radii 0 -> maxRadius 1920) and at radii 10-120 - no accumulator cell reaches 100 votes there, so these time
Canny, points, voting and the centre scan only; buoy frame 3 at dp 2, param2 40, radii 0 and 10-120, which has centres and circles and
so runs every kernel; and a noise frame at a low param2 (tens of thousands of supported circles: the quadratic rank and the sequential
overlap pass).  Prints one line per figure.
--quick: fewer repetitions, no CPU baseline (for a kernel trace)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cuauv-vision-pipeline_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402,F401  (HIP runtime shared with libvp)
from vision import _vp  # noqa: E402
from vision.devmat import DeviceMat  # noqa: E402

import frames as F  # noqa: E402

W, H = 1920, 1080
QUICK = "--quick" in sys.argv


def timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def main():
    ctx = _vp.default_context()
    L = _vp.lib()
    reps = 5 if QUICK else 30
    buoy0 = np.ascontiguousarray(F.s1_buoy(0, W, H)[:, :, 1])
    buoy3 = np.ascontiguousarray(F.s1_buoy(3, W, H)[:, :, 1])
    noise = np.ascontiguousarray(F.s3_noise(0, W, H)[:, :, 1])
    cap = 1 << 20
    out = np.empty((cap, 3), np.float32)
    n = _vp.C.c_int(0)
    cases = (("buoy 0, defaults (dp 1, minDist 20, 100 / 100, radii 0)", buoy0, (1.0, 20.0, 100.0, 100.0, 0, 0), True),
             ("buoy 0, radii 10-120 (dp 1, minDist 20, 100 / 100)", buoy0, (1.0, 20.0, 100.0, 100.0, 10, 120), True),
             ("buoy 3, dp 2, minDist 30, 100 / 40, radii 0", buoy3, (2.0, 30.0, 100.0, 40.0, 0, 0), False),
             ("buoy 3, dp 2, minDist 30, 100 / 40, radii 10-120", buoy3, (2.0, 30.0, 100.0, 40.0, 10, 120), True),
             ("noise, dp 1, minDist 2, 100 / 3, radii 0-12", noise, (1.0, 2.0, 100.0, 3.0, 0, 12), False))
    for label, img, args, cpu in cases:
        dm = DeviceMat.from_host(ctx, img)

        def cabi():
            _vp.check(L.vp_hough_circles_dev(ctx.handle, dm.dev_ptr, W, W, H, *args, _vp.ptr(out), cap, _vp.C.byref(n)), ctx.handle)
        ms_c = timed(cabi, reps)
        circles = n.value
        ctx.set_option(_vp.OPT_HOUGH_CIRCLES_LDS, 0)
        ms_g = timed(cabi, reps)
        ctx.set_option(_vp.OPT_HOUGH_CIRCLES_LDS, 1)
        print(f"1080p {label}: {circles} circles, C-ABI {ms_c:.3f} ms (histograms in device memory {ms_g:.3f} ms)")
        if cpu and not QUICK:
            import hough_circles_restate as HC
            t0 = time.perf_counter()
            ref = HC.hough_circles(img, *args)
            ms_cpu = 1e3 * (time.perf_counter() - t0)
            got = out[None, :circles] if circles else None
            assert (ref is None and got is None) or (ref is not None and got is not None and np.array_equal(ref.view(np.uint32), got.view(np.uint32))), \
                "GPU circles differ from the statement"
            print(f"1080p {label}: CPU statement (numpy, one core) {ms_cpu:.1f} ms, identical circles")


if __name__ == "__main__":
    main()
