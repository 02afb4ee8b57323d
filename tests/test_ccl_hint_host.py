"""The rule that chooses between the crowded-frame kernels (FULL) and the one stand-in launch (LEAN) behind the merge of the two-level
labelling (csrc/vp_ccl_hint.h), compiled for the host under the address and undefined-behaviour sanitizers
(tests/native/ccl_hint_main.cpp) and driven through its transitions: a new context starts LEAN; a hint above 0 gives FULL at once;
31 hints of 0 in a row stay FULL and the 32nd gives LEAN; a hint above 0 in between restarts the count; more than one chain stream
gives FULL always; both overrides work.  CPU only."""
import os
import shutil
import subprocess


def _modes(line):
    name, *cells = line.split()
    return name, "".join(c.split(":")[1] for c in cells)


def test_hint_transitions_under_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the sanitizer build"
    exe = str(tmp_path / "ccl_hint")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I" + os.path.join(root, "cuauv-vision-pipeline_amd", "csrc"), os.path.join(root, "tests", "native", "ccl_hint_main.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, timeout=300)
    err = run.stderr.decode(errors="replace")
    assert "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    assert run.returncode == 0, (run.returncode, err[-2000:])
    lines = run.stdout.decode().splitlines()
    assert lines[0] == "quiet=32 lean=0 full=1"
    got = dict(_modes(l) for l in lines[1:])
    assert got == {
        "start": "LLL",
        "hint_gives_full_at_once": "LFF",
        "quiet_32": "F" + "F" * 31 + "L" + "L",                           # calls 2..32 read the quiet hints 1..31, call 33 the 32nd
        "restart": "F" + "F" * 20 + "F" + "F" * 31 + "L" + "L",
        "two_streams": "FFFF",
        "two_streams_forced_lean": "FFFF",
        "forced_full": "FFFF",
        "forced_lean": "LLLL",
        "override_then_auto": "LF",
    }
