"""Worker of tests/test_gpu_morph_dispatch.py::test_fallback_kernels_on_the_common_shapes: a fresh process, so that libvp reads
VP_NO_SYM / VP_MORPH_STRIP32 from its environment (it reads them once), runs morph_cases.fallback_cases against the oracle, prints
each case as it passes and exits non-zero at the first mismatch."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "cuauv-vision-pipeline_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: F401,E402  -- before libvp: both share the HIP runtime torch ships

import morph_cases as MC  # noqa: E402
from oracle import oracle  # noqa: E402
from vision import _vp  # noqa: E402

assert os.environ.get("VP_NO_SYM") or os.environ.get("VP_MORPH_STRIP32"), "nothing to test: neither switch is set"
oracle.lib()
_vp.lib()
_vp.default_context()
n = 0
try:
    for case in MC.fallback_cases(oracle):
        n += 1
        print("ok", case, flush=True)
except AssertionError as e:
    print("MISMATCH", e, flush=True)
    sys.exit(1)
print("DONE", n, flush=True)
