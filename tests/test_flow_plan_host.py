"""The optical-flow plan (csrc/vp_flow_plan.h: refusals, the rule that says which pyramid levels exist, the index reflection every image
read goes through, the LDS layout of one point) swept on the host under the address and undefined-behaviour sanitizers
(tests/native/flow_plan_main.cpp): every window side 3..63, image sides round every level boundary, maxLevel 0..15; it asserts the level
rule, the LDS regions and their limit, and that every reflected index lies within its level for the extreme positions the range test
admits, and exits non-zero at the first that breaks.  CPU only."""
import os
import re
import shutil
import subprocess


def test_plan_invariants_hold_over_the_sweep_under_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the sanitizer build"
    exe = str(tmp_path / "flow_plan")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I" + os.path.join(root, "cuauv-vision-pipeline_amd", "csrc"), os.path.join(root, "tests", "native", "flow_plan_main.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, timeout=300)
    out, err = run.stdout.decode(errors="replace"), run.stderr.decode(errors="replace")
    assert "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    assert run.returncode == 0 and "FAILED" not in out, (run.returncode, out[-2000:], err[-2000:])
    m = re.fullmatch(r"plans (\d+) levels (\d+) indices (\d+) refused (\d+) max_lds (\d+) limit (\d+)\n", out)
    assert m, out[-500:]
    plans, levels, indices, refused, max_lds, limit = map(int, m.groups())
    assert plans > 10000 and levels > 2 * plans and indices > 1000000 and refused > 100, "the sweep misses a kind of plan"
    assert max_lds <= 65536 < limit == 160 * 1024, "a point's LDS stays below what a kernel gets without asking"
    assert max_lds == (66 * 66 + 64 * 64 * 4 + 63 * 63 * 6 + 3) // 4 * 4, "the 63 x 63 window was swept"
