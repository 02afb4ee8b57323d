"""Worker of tests/test_gpu_ccl_capacity.py::test_tuned_plans_in_a_fresh_process: a fresh process, so that libvp reads the one
labelling tuning under test from its environment (ccl_tuning_from_env is read once), runs ccl_cases.tuned_cases(<setting>) against the
oracle - both numberings; on the two-level path with the crowded-frame kernels forced and with the stand-in launch forced - prints
each case as it passes and exits non-zero at the first mismatch."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "cuauv-vision-pipeline_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: F401,E402  -- before libvp: both share the HIP runtime torch ships

import ccl_cases as CC  # noqa: E402
from oracle import oracle  # noqa: E402
from vision import _vp  # noqa: E402

setting = sys.argv[1]
name, value = setting.split("=")
assert os.environ.get(name) == value, "nothing to test: %s is not set" % setting
assert [k for k in CC.TUNING_NAMES if k in os.environ] == [name], "another labelling tuning is set"
oracle.lib()
_vp.lib()
ctx = _vp.default_context()
n = 0
try:
    for t in CC.tuned_cases(setting):
        ctx.set_option(_vp.OPT_CCL_LEVELS, t.levels)
        ctx.set_option(_vp.OPT_CCL_MERGE_CAP, t.mcap)
        for mode in ((CC.FULL, CC.LEAN) if t.levels == 2 else (CC.AUTO,)):
            ctx.set_option(_vp.OPT_CCL_CROWDED, mode)
            for numbering in (_vp.CCL_BLOCK2X2, _vp.CCL_PIXEL):
                try:
                    if len(t.masks) == 1:
                        CC.check_one(_vp, ctx, oracle, t.masks[0], numbering, t.max_labels)
                    else:
                        CC.check_batch(_vp, oracle, t.masks, numbering, t.max_labels)
                except AssertionError as e:
                    raise AssertionError("%s, levels %d, merge capacity %d, crowded %d, numbering %d: %s" % (t.name, t.levels, t.mcap, mode, numbering, e)) from None
        n += 1
        print("ok", t.name, "levels", t.levels, flush=True)
except AssertionError as e:
    print("MISMATCH", e, flush=True)
    sys.exit(1)
ctx.synchronize()
print("DONE", n, flush=True)
