"""The bit-plane morphology plan (csrc/vp_morph_plan.h: stages, kernel and strip height per launch, LDS bytes, the grouping into
launches and the bit plane each one reads and writes) enumerated on the host under the address and undefined-behaviour sanitizers
(tests/native/morph_plan_main.cpp asserts the properties per case), and its table of switch widths compared byte for byte with
tests/golden/morph_plan.txt, from which the GPU tests take their widths (tests/morph_cases.py).  CPU only."""
import os
import shutil
import subprocess

import morph_cases as MC


def test_plan_holds_its_properties_and_matches_the_table_under_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the sanitizer build"
    exe = str(tmp_path / "morph_plan")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I" + os.path.join(root, "cuauv-vision-pipeline_amd", "csrc"), os.path.join(root, "tests", "native", "morph_plan_main.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, timeout=300)
    err = run.stderr.decode(errors="replace")
    assert "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    assert run.returncode == 0, (run.returncode, err[-4000:])
    want = open(os.path.join(root, "tests", "golden", "morph_plan.txt"), "rb").read()
    assert len(want.splitlines()) == 66
    if run.stdout != want:
        got_l, want_l = run.stdout.decode().splitlines(), want.decode().splitlines()
        bad = [(g, w) for g, w in zip(got_l, want_l) if g != w]
        assert not bad and len(got_l) == len(want_l), (len(got_l), len(want_l), bad[:3])
    assert run.stdout == want


def test_table_agrees_with_the_figures_the_dispatch_was_documented_with():
    """The switch widths worked out by hand from launch_sym / launch_sym_strip / run_bit_stages before the plan had a header."""
    T = MC.plan_table()
    by_halo = {1: ("erode3", 2432, 7680), 2: ("open3", 2368, 7232), 4: ("open5", 2240, 6528), 8: ("open5+close5", 2048, 5440)}
    for halo, (name, strip64, sym) in by_halo.items():
        assert T[name]["halo"] == 2 * halo and T[name]["strip64_last"] == strip64 and T[name]["sym_last"] == sym, (name, T[name])
    assert T["erode5"]["strip64_last"] == 2368 and T["open3+close3"]["sym_last"] == 6528
    assert MC.plan_case("close71x71", 70, 3840)["launches"] == 2 and MC.plan_case("chain8x21", 40, 3840)["launches"] == 3
    assert MC.plan_case("chain8x21", 40, 3840)["planes"] == "0>2,2>1,1>3"
    assert MC.plan_case("erode5x45", 40, 8192) == "refused" and T["erode5x45"]["accepted_last"] < 8192 - 63
    # the benchmark's headline configuration keeps its instantiation and its 64-row strips
    assert MC.plan_case("open5+close5", 1080, 1920)["kernels"] == "sym<3,2,4,2,2>/strip64/lds38400"
    assert MC.plan_case("open5+close5", 2160, 3840)["kernels"] == "sym<3,2,4,2,2>/strip32/lds46080"


def test_the_widths_come_from_the_plan_table():
    """what tests/test_gpu_morph_dispatch.py parametrises over: both sides of the strip and the kernel switch of every halo"""
    assert MC.widths_for("erode3") == [2048, 2049, 2112, 2432, 2433, 3840, 7680, 7681, 8192]
    assert set(MC.all_switch_widths()) == {2048, 2049, 2240, 2241, 2368, 2369, 2432, 2433, 5440, 5441, 6528, 6529, 7232, 7233, 7680, 7681}
    for name in list(MC.SINGLE_OPS) + list(MC.CHAIN_PAIRS):
        assert MC.plan_table()[name]["shape"] is not None, name
    for name, _, _, _ in MC.GENERAL_OPS:
        assert MC.plan_table()[name]["shape"] is None, name
