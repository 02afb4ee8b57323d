"""The two min/max exchange lists of csrc/vp_median.hip (md_select9, md_select25) select the median of every input: by the zero-one
principle a network of exchanges that puts the median of every 0/1 input on its output wire does so for every input, and all 2^9 and
2^25 of those are tried here, 64 per machine word."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _network(name):
    txt = open(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc", "vp_median.hip")).read()
    body = re.search(r"u32 %s\(u32\* p\)\s*\{(.*?)return p\[(\d+)\];" % name, txt, re.S)
    assert body, name
    pairs = [(int(a), int(b)) for a, b in re.findall(r"MD_CX\((\d+),\s*(\d+)\)", body.group(1))]
    return pairs, int(body.group(2))


def _check(name, n, exchanges):
    pairs, out = _network(name)
    assert len(pairs) == exchanges and out == n // 2
    assert all(0 <= a < n and 0 <= b < n and a != b for a, b in pairs)
    idx = np.arange(1 << max(n - 6, 0), dtype=np.uint64)            # input number i: wire j carries bit j of i; bits 0..5 live inside a word
    low = [0xAAAAAAAAAAAAAAAA, 0xCCCCCCCCCCCCCCCC, 0xF0F0F0F0F0F0F0F0, 0xFF00FF00FF00FF00, 0xFFFF0000FFFF0000, 0xFFFFFFFF00000000]
    wires = []
    for j in range(n):
        if j < 6:
            wires.append(np.full(idx.shape, low[j], np.uint64))
        else:
            wires.append(np.where((idx >> np.uint64(j - 6)) & np.uint64(1), np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0)))
    ones = np.zeros(idx.shape + (64,), np.uint8)                     # how many wires carry a 1, per input
    for wv in wires:
        ones += np.unpackbits(wv.view(np.uint8).reshape(-1, 8), axis=1, bitorder="little").reshape(-1, 64)
    expect = np.packbits((ones > n // 2).reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).ravel()
    for a, b in pairs:                                              # a <- min (and), b <- max (or)
        wires[a], wires[b] = wires[a] & wires[b], wires[a] | wires[b]
    assert np.array_equal(wires[out], expect), name


def test_median_of_9_network():
    _check("md_select9", 9, 19)


def test_median_of_25_network():
    _check("md_select25", 25, 99)
