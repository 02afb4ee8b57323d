"""cv2.HoughLines on the GPU (csrc/vp_hough.hip): one 1080p device edge image at 2 / 5 % edge density through the C-ABI call alone and
through the mirror (vision.utils.feature.find_lines), LDS-row voting against global atomics, a batch of 128 frames in one call, and the
CPU statement of the tests (tests/hough_restate.py, numpy on one core) as the baseline.  Prints one line per figure.
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
from vision.utils import feature  # noqa: E402

W, H, STEP, THR = 1920, 1080, np.pi / 180, 200
QUICK = "--quick" in sys.argv


def edge_image(seed, density):
    """Noise at `density` plus a dozen straight lines (the lines a detector looks for; their pixels count towards the density)."""
    rng = np.random.default_rng(seed)
    img = ((rng.random((H, W)) < density * 0.9) * 255).astype(np.uint8)
    for _ in range(12):
        x0, y0, x1, y1 = rng.integers(0, W), rng.integers(0, H), rng.integers(0, W), rng.integers(0, H)
        n = max(abs(x1 - x0), abs(y1 - y0)) + 1
        img[np.linspace(y0, y1, n).round().astype(int), np.linspace(x0, x1, n).round().astype(int)] = 255
    return img


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
    reps = 5 if QUICK else 50
    for density in (0.02, 0.05):
        img = edge_image(1, density)
        dm = DeviceMat.from_host(ctx, img)
        cap = 1 << 16
        out = np.empty((cap, 1, 2), np.float32)
        n = _vp.C.c_int(0)

        def cabi():
            _vp.check(L.vp_hough_lines_dev(ctx.handle, dm.dev_ptr, W, W, H, 1.0, STEP, THR, 0.0, np.pi, _vp.ptr(out), cap, _vp.C.byref(n)),
                      ctx.handle)
        ms_c = timed(cabi, reps)
        lines = n.value
        ms_m = timed(lambda: feature.find_lines(dm, 1, STEP, THR), reps)
        ctx.set_option(_vp.OPT_HOUGH_LDS, 0)
        ms_g = timed(cabi, reps)
        ctx.set_option(_vp.OPT_HOUGH_LDS, 1)
        print(f"1080p {density:.0%} edges ({int((img != 0).sum())} px, {lines} lines at threshold {THR}): C-ABI {ms_c:.3f} ms "
              f"(global-atomic voting {ms_g:.3f} ms), find_lines {ms_m:.3f} ms")
        if not QUICK:
            import hough_restate as HR
            t0 = time.perf_counter()
            ref = HR.hough_lines(img, 1, STEP, THR)
            ms_cpu = 1e3 * (time.perf_counter() - t0)
            assert ref is not None and len(ref) == lines and np.array_equal(ref, out[:lines]), "GPU lines differ from the statement"
            print(f"1080p {density:.0%} edges: CPU statement (numpy, one core) {ms_cpu:.1f} ms, identical lines")
    # batch of 128 frames (2 % density), one call
    nb = 32 if QUICK else 128
    frames = np.stack([edge_image(100 + i, 0.02) for i in range(nb)])
    dev = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    cap = 4096
    out = np.empty((nb, cap, 1, 2), np.float32)
    counts = np.empty(nb, np.int32)

    def batch():
        _vp.check(L.vp_hough_lines_batch_dev(ctx.handle, dev.data_ptr(), W, W * H, nb, W, H, 1.0, STEP, THR, 0.0, np.pi, _vp.ptr(out), cap,
                                             _vp.ptr(counts)), ctx.handle)
    ms_b = timed(batch, 3 if QUICK else 10)
    print(f"batch of {nb} 1080p frames at 2 %: {ms_b:.2f} ms per call = {ms_b / nb:.4f} ms per frame, {nb / ms_b * 1e3:.0f} frames/s "
          f"({int(counts.min())}..{int(counts.max())} lines per frame)")


if __name__ == "__main__":
    main()
