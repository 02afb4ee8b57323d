"""The histogram plan (csrc/vp_hist_plan.h: refusals, bin tables, the LDS limits of the histogram and the back-projection, grids, the
window clipping of mean shift) swept on the host under the address and undefined-behaviour sanitizers
(tests/native/hist_plan_main.cpp), which asserts the plan's invariants for every combination of histogram sizes round the limits and
for image sides at the edges, and exits non-zero at the first that breaks.  CPU only."""
import os
import re
import shutil
import subprocess


def test_plan_invariants_hold_over_the_sweep_under_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the sanitizer build"
    exe = str(tmp_path / "hist_plan")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I" + os.path.join(root, "cuauv-vision-pipeline_amd", "csrc"), os.path.join(root, "tests", "native", "hist_plan_main.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, timeout=300)
    out, err = run.stdout.decode(errors="replace"), run.stderr.decode(errors="replace")
    assert "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    assert run.returncode == 0 and "FAILED" not in out, (run.returncode, out[-2000:], err[-2000:])
    m = re.fullmatch(r"admitted (\d+) in_lds (\d+) in_memory (\d+) windows (\d+) max_lds (\d+) limit (\d+)\n", out)
    assert m, out[-500:]
    admitted, in_lds, in_memory, windows, max_lds, limit = map(int, m.groups())
    assert admitted > 3000 and in_lds > 100 and in_memory > 100 and windows > 1000, "the sweep misses a kind of plan"
    assert max_lds <= limit == 160 * 1024
