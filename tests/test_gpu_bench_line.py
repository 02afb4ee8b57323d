"""The contract of bench.py's output as the driver reads it: stdout is ONE line, a JSON object with the keys the round's measurement rules
name (metric, value, roofline, cpu_baseline, ...), whatever the side measurements print (the modules they run announce themselves)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_stdout_is_one_json_line_with_the_contract_keys():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "3", "--warmup", "1", "--regions", "1", "--cpu-seconds", "1"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines[:5]
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
                "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["dtype"] == "u8" and d["vs_baseline"] is None
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["data"] == "synthetic" and "workload" in d["config"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and "traffic" in r
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["cores"] == 1 and c["value"] > 0 and c["sample"]
    for key in ("process_body_red_buoy", "process_body_bins", "runtime_e2e_red_buoy", "runtime_e2e_bins", "host_fed_1080p", "host_fed_4k"):
        assert key in d["extras"], (key, d["extras"].get("runtime_rates_error"))
    assert d["value"] > 0 and abs(d["value"] - 128 * 1e3 / d["ms_per_step"]) / d["value"] < 0.01


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_what_they_computed(oracle, tmp_path):
    """Without --full: one region of exactly --steps steps, the headline keys only (no roofline, cpu_baseline, kernels, extras), and
    --dump-outputs holds what the last step computed - every dumped value equals the oracle's chain on the same synthetic frames."""
    import numpy as np
    import frames as F
    sys.path.insert(0, ROOT)
    import bench
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines[:5]
    d = json.loads(lines[0])
    assert d["metric"] == "frames/sec for color->threshold->morph->CCL at 1080p" and d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert d["dtype"] == "u8" and d["steps"] == 3 and d["warmup"] == 1 and d["regions"] == 1 and len(d["region_ms_per_step"]) == 1
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["kernels"] == {} and d["extras"] == {}
    assert d["value"] > 0 and abs(d["value"] - 128 * 1e3 / d["ms_per_step"]) / d["value"] < 0.01

    files = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sum(a.nbytes for a in files.values()) <= 64 * 10**6 and all(a.dtype in (np.float32, np.float64) for a in files.values())
    B, ML = 128, 256
    refs = [oracle.chain(F.s1_buoy(i, 1920, 1080), oracle.MODE_LAB, (0, 150, 0), (255, 255, 255), [oracle.OPEN, oracle.CLOSE], 5, 5, 2, ML)
            for i in range(8)]                               # the batch tiles these 8 frames
    for name in ("threshed", "cleaned", "labels"):
        assert np.array_equal(files[name + "_frames"], np.stack([refs[0][name], refs[(B - 1) % 8][name]])), name
        pos = bench.sample_positions(B * 1080 * 1920)
        f, px = np.divmod(pos, 1080 * 1920)
        exp = np.stack([r[name].reshape(-1) for r in refs])[f % 8, px]
        assert np.array_equal(files[name + "_sample"], exp), name
    assert np.array_equal(files["nlabels"], [refs[i % 8]["nlabels"] for i in range(B)])
    for i in range(B):
        r = refs[i % 8]
        assert np.array_equal(files["stats"][i][:r["nlabels"]], r["stats"]) and np.array_equal(files["centroids"][i][:r["nlabels"]], r["centroids"]), i
