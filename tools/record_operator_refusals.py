"""Records what the calls of tests/operator_refusal_cases.py raise into tests/golden/operator_refusals.json.

    python tools/record_operator_refusals.py [--root DIR]

Run it on the commit whose refusals are the expectation (the parent of a change to the Python operator layer), never on the change
itself: --root DIR takes the package of another checkout, built there, while the cases and the output stay those of this one.  Needs
no GPU: a case that returns, or that fails for want of a device, is an error of the table."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=HERE)
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path[:0] = [os.path.join(ROOT, "cuauv-vision-pipeline_amd"), os.path.join(HERE, "tests")]

import operator_refusal_cases as cases  # noqa: E402

record = {}
for name, call in cases.cases():
    got = cases.outcome(call)
    assert got is not None, f"{name}: the call was not refused"
    assert got[0] != "VpError" and "vp_create" not in got[1], f"{name}: the call reached the device: {got}"
    assert name not in record, f"{name}: two cases of one name"
    record[name] = got
path = os.path.join(HERE, "tests", "golden", "operator_refusals.json")
with open(path, "w") as fh:
    json.dump(record, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(f"{len(record)} refusals -> {path}")
