"""Worker of tests/test_gpu_balance.py::test_fold_forced_in_a_fresh_process: a fresh process, so that libvp reads VP_CB_FORCE_FOLD from
its environment (it reads it once).  Runs every tiled case of balance_cases and the batch of three against the oracle, checks after
each call that the fold ran for every tile of every frame, prints each case as it passes and exits non-zero at the first mismatch."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "cuauv-vision-pipeline_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: F401,E402  -- before libvp: both share the HIP runtime torch ships

import numpy as np  # noqa: E402

import balance_cases as BC  # noqa: E402
from oracle import oracle  # noqa: E402
from vision import _vp  # noqa: E402
from vision.modules.color_balance import balance  # noqa: E402

assert os.environ.get("VP_CB_FORCE_FOLD") == "1", "nothing to test: VP_CB_FORCE_FOLD is not set"
oracle.lib()
_vp.lib()
_vp.default_context()
FLAGS = (dict(), dict(hsv_contrast_correct=False, rgb_extrema_clipping=False))
n = 0
try:
    for name, f, hb, vb in BC.tiled_cases():
        for kw in FLAGS:
            got = balance(f, horizontal_blocks=hb, vertical_blocks=vb, **kw)
            folds = BC.last_folds(_vp)
            assert folds == hb * vb, (name, kw, "tiles folded", folds, "expected", hb * vb)
            BC.assert_exact(got, oracle.color_balance(f, horizontal_blocks=hb, vertical_blocks=vb, mean_mode=0, **kw), (name, kw))
            n += 1
            print("ok", name, kw, flush=True)
    frames = BC.batch_frames()
    for hb, vb in BC.BATCH_TILINGS[1:]:
        for in_place, kw in zip((False, True), FLAGS):
            rc, got, back, guard = BC.run_dev(_vp, frames, BC.flag_bits(_vp, **kw), hb, vb, in_place)
            folds = BC.last_folds(_vp)
            assert rc == _vp.OK, ("batch", hb, vb, kw, rc)
            assert folds == len(frames) * hb * vb, ("batch", hb, vb, kw, "tiles folded", folds, "expected", len(frames) * hb * vb)
            for k, f in enumerate(frames):
                BC.assert_exact(got[k], oracle.color_balance(f, horizontal_blocks=hb, vertical_blocks=vb, mean_mode=0, **kw), ("batch", hb, vb, kw, k))
            assert (guard == BC.FILL).all() and (in_place or np.array_equal(back, frames)), ("batch", hb, vb, kw, "guard or source written")
            n += 1
            print("ok batch", hb, vb, kw, flush=True)
    name, f, hb, vb = BC.tiled_cases()[0]
    got = balance(f, equalize_rgb=False, horizontal_blocks=hb, vertical_blocks=vb)      # the means are not read: nothing to fold
    folds = BC.last_folds(_vp)
    assert folds == 0, (name, "equalize_rgb=False", "tiles folded", folds)
    BC.assert_exact(got, oracle.color_balance(f, equalize_rgb=False, mean_mode=0), (name, "equalize_rgb=False"))
    n += 1
    print("ok", name, "equalize_rgb=False", flush=True)
except AssertionError as e:
    print("MISMATCH", e, flush=True)
    sys.exit(1)
print("DONE", n, flush=True)
