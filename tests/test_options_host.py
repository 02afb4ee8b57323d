"""The options table (csrc/vp_options.h: range, default and environment override of every VP_OPT_*) driven on the host under the
address and undefined-behaviour sanitizers (tests/native/options_main.cpp) and compared with the table written out below, which is
the one include/vp.h documents.  CPU only."""
import os
import shutil
import subprocess

INT_MAX = 2**31 - 1
# id, name, min, max, default, environment variable
ROWS = [
    (1, "CHAIN_STREAMS", 1, 4, 1, "VP_CHAIN_STREAMS"),
    (2, "CCL_LEVELS", 1, 2, 2, "VP_CCL_LEVELS"),
    (3, "CCL_MERGE_CAP", -1, INT_MAX, -1, None),
    (4, "FLAT_OPS", 0, 1, 1, None),
    (5, "HOUGH_LDS", 0, 1, 1, None),
    (6, "HOUGH_CIRCLES_LDS", 0, 1, 1, None),
    (7, "BLUR_ONEPASS", -1, 1, -1, None),
    (8, "MEDIAN_MASK", -1, 1, -1, "VP_OPT_MEDIAN_MASK"),
    (9, "CLAHE_SPLIT", 0, 64, 0, "VP_OPT_CLAHE_SPLIT"),
    (10, "CCL_CROWDED", 0, 2, 0, "VP_OPT_CCL_CROWDED"),
    (11, "LABEL_MOMENTS_LDS", -1, 1, -1, None),
]
# per named variable: an in-range text, an out-of-range text, and what atoi("abc") = 0 leaves in the option
ENV_CASES = {
    "VP_CHAIN_STREAMS": ("3", "5", 1),        # 0 is below the range: the default stays
    "VP_CCL_LEVELS": ("1", "3", 2),
    "VP_OPT_MEDIAN_MASK": ("1", "2", 0),      # 0 is a value of the option
    "VP_OPT_CLAHE_SPLIT": ("64", "65", 0),
    "VP_OPT_CCL_CROWDED": ("2", "-1", 0),
}


def _expected():
    defaults = {r[0]: r[4] for r in ROWS}

    def all_line(tag, over=None):
        vals = {**defaults, **(over or {})}
        return tag + " " + " ".join(str(vals[i]) for i in range(1, 12))

    lines = ["count=12"]
    for oid, _name, lo, hi, dflt, env in ROWS:
        parts = ["row %d default=%d env=%s" % (oid, dflt, env or "-")]
        for value, ok in ((lo - 1, False), (lo, True), (hi, True), (hi + 1, False)):
            if value > INT_MAX or value < -2**31:
                parts.append("-")
            else:
                parts.append("%d:%s:%d" % (value, "A" if ok else "R", value if ok else dflt))
        lines.append(" ".join(parts))
    for oid in (0, 12, 77, -1):
        lines.append("id %d R changed=0" % oid)
    lines.append(all_line("env none:"))
    by_env = {r[5]: r[0] for r in ROWS if r[5]}
    assert sorted(by_env) == sorted(ENV_CASES)
    for oid, _name, _lo, _hi, dflt, env in ROWS:
        if not env:
            continue
        good, bad, after_abc = ENV_CASES[env]
        lines.append(all_line("env %s=%s:" % (env, good), {oid: int(good)}))
        lines.append(all_line("env %s=%s:" % (env, bad)))
        lines.append(all_line("env %s=abc:" % env, {oid: after_abc}))
    lines.append(all_line("env VP_OPT_FLAT_OPS=0:"))
    return lines


def test_options_table_under_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the sanitizer build"
    exe = str(tmp_path / "options")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I" + os.path.join(root, "cuauv-vision-pipeline_amd", "csrc"), os.path.join(root, "tests", "native", "options_main.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-2000:]
    assert "warning" not in build.stderr, build.stderr[-2000:]
    env = {k: v for k, v in os.environ.items() if k not in ENV_CASES}   # the program passes its own getenv; the real one is not consulted
    run = subprocess.run([exe], capture_output=True, env=env, timeout=300)
    err = run.stderr.decode(errors="replace")
    assert "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    assert run.returncode == 0, (run.returncode, err[-2000:])
    got, want = run.stdout.decode().splitlines(), _expected()
    assert len(want) == 1 + 11 + 4 + 1 + 15 + 1
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad and len(got) == len(want), (len(got), len(want), bad[:3])

