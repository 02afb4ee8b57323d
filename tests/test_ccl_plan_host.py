"""The labelling plan (csrc/vp_ccl_plan.h: path, strips, LDS per kernel and instantiation for a frame size) computed on the host under
the address and undefined-behaviour sanitizers (tests/native/ccl_plan_main.cpp) and compared byte for byte with
tests/golden/ccl_plan.txt, which was recorded from the dispatcher before the plan was moved out of it.  CPU only."""
import os
import shutil
import subprocess

_TUNING = ("VP_C3_IDS", "VP_CCL3", "VP_C3_LGRID", "VP_C3_BGRID", "VP_C3_AGRID", "VP_C3_AGRID_LIGHT", "VP_CL_ROWS", "VP_CL_CAP")


def test_plan_matches_recorded_dispatch_under_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the sanitizer build"
    exe = str(tmp_path / "ccl_plan")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I" + os.path.join(root, "cuauv-vision-pipeline_amd", "csrc"), os.path.join(root, "tests", "native", "ccl_plan_main.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-2000:]
    env = {k: v for k, v in os.environ.items() if k not in _TUNING}
    run = subprocess.run([exe], capture_output=True, env=env, timeout=300)
    err = run.stderr.decode(errors="replace")
    assert "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    assert run.returncode == 0, (run.returncode, err[-2000:])
    want = open(os.path.join(root, "tests", "golden", "ccl_plan.txt"), "rb").read()
    assert len(want.splitlines()) == 174      # 86 recorded from the dispatcher + the shapes and settings of tests/ccl_cases.py
    if run.stdout != want:
        got_l, want_l = run.stdout.decode().splitlines(), want.decode().splitlines()
        bad = [(g, w) for g, w in zip(got_l, want_l) if g != w]
        assert not bad and len(got_l) == len(want_l), (len(got_l), len(want_l), bad[:3])
    assert run.stdout == want
