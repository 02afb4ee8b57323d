"""tests/ccl_cases.py without a GPU: its restatement of the labelling plan (strip geometry, cap2, the one-level capacity, the
crowded-frame plan) against every line of tests/golden/ccl_plan.txt - which tests/test_ccl_plan_host.py pins to csrc/vp_ccl_plan.h -
and every mask the GPU tests use, built here once so that each builder's own assertion (the oracle's count of the strip's components,
the word-segment count, which side of the capacity the mask lies on) has run on the reference alone."""
import os

import numpy as np
import pytest

import ccl_cases as CC

_FIELDS = ("rows", "ww", "wb", "strips", "cap2", "rc", "tail_words", "lds2", "two_level", "mcap", "R3", "strips3", "ids3", "ok3", "cap1")


def _golden():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ccl_plan.txt")
    for line in open(path):
        key, val = line.split(" : ")
        k = dict(x.split("=", 1) for x in key.split())
        yield k["env"], int(k["h"]), int(k["w"]), int(k["levels"]), int(k["mcap_in"]), {a: int(b) for a, b in (x.split("=") for x in val.split())}


def test_restated_plan_matches_every_golden_line():
    n = 0
    for env, h, w, levels, mcap_in, want in _golden():
        got = CC.plan(h, w, levels, mcap_in, env)
        assert {f: got[f] for f in _FIELDS} == {f: want[f] for f in _FIELDS}, (env, h, w, levels, mcap_in)
        assert CC.geom(h, w, env) == (want["rows"], want["ww"], want["wb"]) and CC.cap2(h, w, env) == want["cap2"] and CC.cap1(h, w, env) == want["cap1"]
        if want["two_level"] and w <= 4096:
            R, strips3, ids, ok = CC.c3_make_plan(h, w, min(CC.tuning(env)["c3_ids"], CC.C3_IDS), env)
            assert (R, strips3, ids) == (want["R3"], want["strips3"], want["ids3"]) and ok >= want["ok3"]
        n += 1
    assert n == 174


def test_every_shape_and_setting_of_the_cases_is_in_the_golden_file():
    lines = {(env, h, w, levels) for env, h, w, levels, _, _ in _golden()}
    for h, w in ((65, 200), (65, 64), (40, 2112), (704, 200), (64, 200), (64, 400), (64, 640), (8192, 64), (8193, 64)):
        assert ("-", h, w, 1) in lines and ("-", h, w, 2) in lines
    for env in CC.TUNED_SETTINGS:
        for t in CC.tuned_cases(env):
            h, w = t.masks[0].shape
            assert (env, h, w, t.levels) in lines, (env, h, w, t.levels)


def test_constants_are_the_headers():
    assert (CC.RC, CC.CL_ROWS, CC.C2_MCAP, CC.C2_MAXSTRIPS) == (96, 32, 2048, 256)
    assert (CC.C3_IDS, CC.C3_ACC, CC.C3_LIGHT_ROOTS, CC.C3_LIGHT_ACC, CC.C3_MAX_STRIPS) == (16384, 2304, 1024, 768, 512)
    assert tuple(CC.TUNING_NAMES) == __import__("test_ccl_plan_host")._TUNING


def test_counters():
    m = np.zeros((40, 130), np.uint8)
    m[0, 60:70] = 255                   # one run over a word boundary: two segments, one component
    m[2, 0] = m[2, 2] = 255             # two pixels, two apart: two components
    m[31, 100] = m[32, 101] = 255       # a diagonal contact across the boundary of 32-row strips: one component in each strip
    assert CC.segments(m[:1]) == 2 and CC.strip_segments(m, 32) == [5, 1]
    assert CC.strip_components(m, 32) == [4, 1] and CC.c3_local_roots(m, 8) == [3, 0, 0, 1, 1]
    assert CC.handed_over(m) is False and CC.handed_over(m, mcap_in=4) is True and CC.handed_over(m, levels=1) is None


def _strip_counts(c, env=None):
    rows = CC.geom(*c.mask.shape, env)[0]
    return max(CC.strip_components(c.mask, rows)), max(CC.strip_segments(c.mask, rows)), sum(CC.strip_components(c.mask, rows))


def test_rc_masks():
    cs = CC.rc_cases()
    assert [c.handed for c in cs] == [False, False, True] * 3 + [False, True]
    assert [_strip_counts(c)[0] for c in cs] == [CC.RC - 1, CC.RC, CC.RC + 1] * 3 + [CC.RC, CC.RC + 1]
    assert all(_strip_counts(c)[1] <= CC.cap2(65, 200) and _strip_counts(c)[2] <= CC.C2_MCAP for c in cs)     # rc alone decides


@pytest.mark.parametrize("h,w,strips", [(65, 200, (1, 0)), (65, 64, (1, 0)), (40, 2112, (1,))])
def test_cap2_masks(h, w, strips):
    cs = CC.cap_cases(h, w, strips=strips)
    cap = CC.cap2(h, w)
    assert cap == {(65, 200): 130, (65, 64): 34, (40, 2112): 530}[(h, w)] and CC.geom(h, w)[0] == (16 if w == 2112 else 32)
    assert [_strip_counts(c)[1] for c in cs] == [cap - 1, cap, cap + 1] * len(strips)
    assert [c.handed for c in cs] == [False, False, True] * len(strips)
    assert all(_strip_counts(c)[0] <= 5 for c in cs)                                                          # cap2 alone decides


def test_merge_capacity_masks():
    for cs, cap in ((CC.mcap_small_cases(), CC.MCAP_SMALL), (CC.mcap_default_cases(), CC.C2_MCAP)):
        assert [_strip_counts(c)[2] for c in cs] == [cap - 1, cap, cap + 1] and [c.handed for c in cs] == [False, False, True]
        assert all(_strip_counts(c)[0] <= CC.RC and _strip_counts(c)[1] <= CC.cap2(*c.mask.shape) for c in cs)
    assert CC.mcap_default_cases()[0].mask.shape == (704, 200) and CC.plan(704, 200)["strips"] == 22
    assert all(c.max_labels > 2100 for c in CC.mcap_default_cases())


def test_crowded_frame_masks():
    assert CC.c3_make_plan(64, 200) == (32, 2, 3200, 1) and CC.c3_make_plan(64, 400) == (32, 2, 6400, 1) and CC.c3_make_plan(64, 640) == (32, 2, 10240, 1)
    for cs, counts in ((CC.light_heavy_cases(), [CC.C3_LIGHT_ROOTS - 1, CC.C3_LIGHT_ROOTS, CC.C3_LIGHT_ROOTS + 1]),
                       (CC.light_acc_cases(), [CC.C3_LIGHT_ACC - 1, CC.C3_LIGHT_ACC, CC.C3_LIGHT_ACC + 1]),
                       (CC.heavy_acc_cases(), [CC.C3_ACC - 1, CC.C3_ACC, CC.C3_ACC + 1, 2 * CC.C3_ACC + 1])):
        assert [CC.c3_local_roots(c.mask, 32) for c in cs] == [[k, 40] for k in counts]
        assert all(c.handed for c in cs)
    assert CC.C3_LIGHT_ACC < CC.C3_LIGHT_ROOTS < 2 * CC.C3_LIGHT_ACC       # the LIGHT instantiation: at most two passes
    assert CC.C3_LIGHT_ROOTS < CC.C3_ACC - 1                               # so every mask around C3_ACC is labelled by HEAVY


def test_strip_count_masks():
    a, b = CC.maxstrips_cases()
    assert a.mask.shape == (8192, 64) and b.mask.shape == (8193, 64)
    assert (CC.plan(8192, 64)["strips"], CC.plan(8192, 64)["two_level"], CC.plan(8193, 64)["strips"], CC.plan(8193, 64)["two_level"]) == (256, 1, 257, 0)
    assert a.handed is False and b.handed is None


@pytest.mark.parametrize("env", CC.TUNED_SETTINGS)
def test_tuned_masks(env):
    cases = CC.tuned_cases(env)
    assert cases and all(m.dtype == np.uint8 and len({x.shape for x in t.masks}) == 1 for t in cases for m in t.masks)
    if env.startswith("VP_CL_ROWS"):
        rows = int(env.split("=")[1])
        segs = sorted({max(CC.strip_segments(t.masks[0], rows)) for t in cases if t.name.startswith("cap") and t.masks[0].shape == (65, 200)})
        assert segs == [CC.cap2(65, 200, env) + d for d in (-1, 0, 1)] == [rows * 4 + 2 + d for d in (-1, 0, 1)]
        comps = sorted({max(CC.strip_components(t.masks[0], rows)) for t in cases if t.name.startswith("rc")})
        assert comps == [CC.RC - 1, CC.RC, CC.RC + 1] and {t.levels for t in cases} == {1, 2}
