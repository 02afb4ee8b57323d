"""The feature plans (csrc/vp_features_plan.h: refusals, the FAST tiles and raster chunks, the describe grid, both workspaces, the
matcher's query tiles and train splits, the pattern rule) swept on the host under the address and undefined-behaviour sanitizers
(tests/native/features_plan_main.cpp): image sides round every tile boundary, row counts round every block, split and cap boundary.  It
asserts that every grid and workspace region is positive and fits, that the splits cover every train row exactly once, and that the
steered pattern stays within 15 of the point; it exits non-zero at the first that breaks.  CPU only."""
import os
import re
import shutil
import subprocess


def test_plan_invariants_hold_over_the_sweep_under_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the sanitizer build"
    exe = str(tmp_path / "features_plan")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I" + os.path.join(root, "cuauv-vision-pipeline_amd", "csrc"), os.path.join(root, "tests", "native", "features_plan_main.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-2000:]
    assert "warning" not in build.stderr, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, timeout=300)
    out, err = run.stdout.decode(errors="replace"), run.stderr.decode(errors="replace")
    assert "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    assert run.returncode == 0 and "FAILED" not in out, (run.returncode, out[-2000:], err[-2000:])
    m = re.fullmatch(r"fast (\d+) describe (\d+) hamming (\d+) refused (\d+) split_plans (\d+) max_splits (\d+) max_partial (\d+) pattern_reach (\d+)\n", out)
    assert m, out[-500:]
    fast, describe, hamming, refused, split_plans, max_splits, max_partial, reach = map(int, m.groups())
    assert fast > 1000 and describe > 1000 and hamming > 5000 and refused > 1000, "the sweep misses a kind of plan"
    assert split_plans > 500 and 2 <= max_splits <= 512, "no plan that splits the train set was swept"
    assert 0 < max_partial <= 8 << 20 and reach <= 15
