"""The labelling on the two sides of every capacity that a count found on the device is compared with: rc components and cap2 word
segments per strip (k_ccl2_local), the merge capacity (k_ccl2_merge), the roots the LIGHT instantiation of k_ccl3_label takes, the
accumulator passes of both instantiations, the strip counts of the two-level path and of the crowded-frame kernels, and the
environment tunings of the plan.  The masks come from tests/ccl_cases.py, whose builders assert every count on the CPU
(tests/test_ccl_cases.py runs them all without a GPU); the capacities are read from csrc/vp_ccl_plan.h.  Every output - labels,
nlabels, stats, centroids, the rows past the last label - is compared bitwise with the oracle's, in both numberings, under the four
configurations of tests/test_gpu_ccl_levels.py, and with either form of finishing a handed-over frame forced."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ccl_cases as CC
from test_gpu_ccl_levels import CONFIGS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [("auto", CC.AUTO), ("lean", CC.LEAN), ("full", CC.FULL)]


@pytest.fixture(params=CONFIGS, ids=[c[0] for c in CONFIGS])
def config(vp, request):
    ctx = vp.default_context()
    name, levels, cap = request.param
    ctx.set_option(vp.OPT_CCL_LEVELS, levels)
    ctx.set_option(vp.OPT_CCL_MERGE_CAP, cap)
    ctx.config_name = name
    yield ctx
    ctx.synchronize()
    ctx.set_option(vp.OPT_CCL_LEVELS, 2)
    ctx.set_option(vp.OPT_CCL_MERGE_CAP, -1)
    ctx.set_option(vp.OPT_CCL_CROWDED, CC.AUTO)


@pytest.fixture(params=MODES, ids=[m[0] for m in MODES])
def crowded(request):
    return request.param[1]


def _run(vp, ctx, oracle, cases, modes):
    for mode in modes:
        ctx.set_option(vp.OPT_CCL_CROWDED, mode)
        for c in cases:
            for numbering in (vp.CCL_BLOCK2X2, vp.CCL_PIXEL):
                try:
                    CC.check_one(vp, ctx, oracle, c.mask, numbering, c.max_labels)
                except AssertionError as e:
                    raise AssertionError(f"{c.name}, crowded {mode}, numbering {numbering}: {e}") from None


def test_rc_components_in_a_strip(vp, oracle, config, crowded):
    """rc - 1, rc, rc + 1 components in the middle, the first and the last (one-row) strip of 65 x 200 with a blob through or into the
    strip, and rc / rc + 1 of which ten are bars that continue into both neighbours."""
    _run(vp, config, oracle, CC.rc_cases(), [crowded])


@pytest.mark.parametrize("h,w,strips", [(65, 200, (1, 0)), (65, 64, (1, 0)), (40, 2112, (1,))], ids=["65x200", "65x64", "40x2112"])
def test_cap_segments_in_a_strip(vp, oracle, config, crowded, h, w, strips):
    """cap2 - 1, cap2, cap2 + 1 word segments in a strip of two components: the LDS union-find of k_ccl2_local exactly full and one
    beyond; the same masks are at the capacity of the one-level k_ccl_local in the "one-level" configuration.  40 x 2112: strips of 16
    rows, 33 words per row."""
    assert ("one-level", 1, -1) in CONFIGS
    _run(vp, config, oracle, CC.cap_cases(h, w, strips=strips), [crowded])
    # the path, from the launches of the last call: local, boundary, rank, stats, final, write on the one-level kernels; local, merge,
    # one stand-in or six crowded-frame launches, write on the two-level path
    n = config.ccl_last_launches()
    assert n == (6 if config.config_name == "one-level" else {CC.FULL: 9, CC.LEAN: 4}.get(crowded, n)) and n in (4, 6, 9)


def test_merge_capacity_at_its_default(vp, oracle, config, crowded):
    """C2_MCAP - 1, C2_MCAP, C2_MCAP + 1 strip components in the 22 strips of 704 x 200, no strip above rc: three masks that differ in one
    pixel, the last list entry the merge block's LDS holds and the first it does not."""
    _run(vp, config, oracle, CC.mcap_default_cases(), [crowded])


@pytest.mark.parametrize("mode", [m[1] for m in MODES], ids=[m[0] for m in MODES])
def test_merge_capacity_through_the_option(vp, oracle, mode):
    """VP_OPT_CCL_MERGE_CAP = 6 and frames of 5, 6 and 7 strip components: in one batch through vp_chain_run beside an empty and a full
    frame, and one by one."""
    ctx = vp.default_context()
    cases = CC.mcap_small_cases()
    masks = [cases[2].mask, np.zeros((65, 200), np.uint8), cases[0].mask, cases[1].mask, np.full((65, 200), 255, np.uint8), cases[2].mask]
    ctx.set_option(vp.OPT_CCL_MERGE_CAP, CC.MCAP_SMALL)
    ctx.set_option(vp.OPT_CCL_CROWDED, mode)
    try:
        for numbering in (vp.CCL_BLOCK2X2, vp.CCL_PIXEL):
            CC.check_batch(vp, oracle, masks, numbering)
        _run(vp, ctx, oracle, cases, [mode])
    finally:
        ctx.synchronize()
        ctx.set_option(vp.OPT_CCL_MERGE_CAP, -1)
        ctx.set_option(vp.OPT_CCL_CROWDED, CC.AUTO)


@pytest.fixture(params=[0, -1], ids=["cap0", "default cap"])
def handing_over(vp, request):
    ctx = vp.default_context()
    ctx.set_option(vp.OPT_CCL_LEVELS, 2)
    ctx.set_option(vp.OPT_CCL_MERGE_CAP, request.param)
    yield ctx
    ctx.synchronize()
    ctx.set_option(vp.OPT_CCL_MERGE_CAP, -1)
    ctx.set_option(vp.OPT_CCL_CROWDED, CC.AUTO)


def test_light_and_heavy_strips(vp, oracle, handing_over):
    """C3_LIGHT_ROOTS - 1, C3_LIGHT_ROOTS, C3_LIGHT_ROOTS + 1 local roots in the first crowded-frame strip of 64 x 200 (R = 32, 3200
    ids), 40 in the second: the last strip k_ccl3_rank gives to the LIGHT instantiation of k_ccl3_label and the first it gives to HEAVY.
    Which instantiation labelled a strip leaves no trace on the host: the evidence that the masks lie on the two sides is the count the
    builder asserted with the oracle (ccl_cases.c3_local_roots; tests/test_ccl_cases.py)."""
    assert CC.c3_make_plan(64, 200) == (32, 2, 3200, 1)
    _run(vp, handing_over, oracle, CC.light_heavy_cases(), [CC.FULL, CC.LEAN])


def test_light_accumulator_passes(vp, oracle, handing_over):
    """C3_LIGHT_ACC - 1, C3_LIGHT_ACC, C3_LIGHT_ACC + 1 local components in a LIGHT strip: one pass over the strip for their statistics,
    and the first component of a second pass.  The number of passes leaves no trace on the host either: the builder's count is the
    evidence."""
    _run(vp, handing_over, oracle, CC.light_acc_cases(), [CC.FULL, CC.LEAN])


def test_heavy_accumulator_passes(vp, oracle, handing_over):
    """C3_ACC - 1, C3_ACC, C3_ACC + 1 local components in a HEAVY strip of 64 x 400 (R = 32, 6400 ids), and 2 * C3_ACC + 1 in 64 x 640
    (10,240 ids: the taller block as well) for the first component of a third pass; evidence as above."""
    assert CC.c3_make_plan(64, 400) == (32, 2, 6400, 1) and CC.c3_make_plan(64, 640) == (32, 2, 10240, 1)
    _run(vp, handing_over, oracle, CC.heavy_acc_cases(), [CC.FULL, CC.LEAN])


@pytest.mark.parametrize("mode", [m[1] for m in MODES], ids=[m[0] for m in MODES])
def test_both_classes_in_one_batch(vp, oracle, mode):
    """LIGHT and HEAVY strips in one frame and in one batch of vp_chain_run: the masks around C3_LIGHT_ROOTS (64 x 200) beside an empty
    frame and a blob frame, and the masks around C3_ACC (64 x 400) likewise."""
    ctx = vp.default_context()
    ctx.set_option(vp.OPT_CCL_CROWDED, mode)
    try:
        for cases in (CC.light_heavy_cases() + CC.light_acc_cases()[1:], CC.heavy_acc_cases()[:3]):
            h, w = cases[0].mask.shape
            masks = [cases[2].mask, np.zeros((h, w), np.uint8), cases[0].mask, CC.blobs(h, w, 0, 32), cases[1].mask] + [c.mask for c in cases[3:]]
            for numbering in (vp.CCL_BLOCK2X2, vp.CCL_PIXEL):
                CC.check_batch(vp, oracle, masks, numbering, max_labels=max(c.max_labels for c in cases))
    finally:
        ctx.synchronize()
        ctx.set_option(vp.OPT_CCL_CROWDED, CC.AUTO)


def test_strip_count_of_the_two_level_path(vp, oracle, config):
    """8192 x 64: C2_MAXSTRIPS strips, resolved by the merge with every strip that holds pixels at cap2; 8193 x 64: one strip more, the
    one-level kernels for the whole call.  300 pixels and a bar through every strip."""
    _run(vp, config, oracle, CC.maxstrips_cases(), [CC.AUTO])


def _was_handed_over(vp, oracle, m, merge_cap=-1, max_labels=None):
    """On a context of its own, in automatic mode: the call after the one that labels m queues the six crowded-frame launches (9 in
    all) when the merge handed m over, and the one stand-in launch (4 in all) when it did not - the hint, tests/test_gpu_ccl_lean.py."""
    ctx = vp.Context(0)
    try:
        ctx.set_option(vp.OPT_CCL_MERGE_CAP, merge_cap)
        CC.check_one(vp, ctx, oracle, m, 2, max_labels)
        assert ctx.ccl_last_launches() == 4
        ctx.set_option(vp.OPT_CCL_MERGE_CAP, -1)
        clean = np.zeros((33, 65), np.uint8)
        clean[5:20, 10:40] = 255
        CC.check_one(vp, ctx, oracle, clean, 2)
        n = ctx.ccl_last_launches()
        assert n in (4, 9), n
        return n == 9
    finally:
        ctx.close()


def test_every_capacity_hands_over_one_above_it(vp, oracle):
    """The path each boundary mask took, from the launch count of the next call: rc - 1, rc, cap2 - 1, cap2, mcap - 1, mcap (at the
    default and through the option) are resolved by the merge, each + 1 is handed over.  Fails when a capacity moves without
    csrc/vp_ccl_plan.h saying so."""
    groups = [(CC.rc_cases(), -1), (CC.cap_cases(65, 200), -1), (CC.cap_cases(65, 64), -1), (CC.cap_cases(40, 2112, strips=(1,)), -1),
              (CC.mcap_default_cases(), -1), (CC.mcap_small_cases(), CC.MCAP_SMALL)]
    seen = []
    for cases, cap in groups:
        for c in cases:
            assert c.handed in (False, True)
            got = _was_handed_over(vp, oracle, c.mask, cap, c.max_labels)
            assert got == c.handed, (c.name, "handed over" if got else "resolved by the merge")
            seen.append(c.handed)
    assert seen.count(True) == 11 and seen.count(False) == 21


@pytest.mark.parametrize("setting", CC.TUNED_SETTINGS)
def test_tuned_plans_in_a_fresh_process(setting):
    """The environment tunings of the labelling plan on the GPU, each in a child of its own (libvp reads them once per process):
    VP_CCL3=0 (handed-over frames finished by the one-level kernels), VP_C3_IDS (crowded-frame strips of 4 and 2 rows; 512 strips and
    the fallback at 513), VP_CL_ROWS (strips of 8 and 16 rows with the rc and cap2 masks rebuilt for them), VP_CL_CAP (the one-level
    capacity at 64 segments)."""
    env = {k: v for k, v in os.environ.items() if k not in CC.TUNING_NAMES}
    name, value = setting.split("=")
    env[name] = value
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_ccl_tuning_worker.py"), setting], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    assert "DONE %d" % len(CC.tuned_cases(setting)) in r.stdout and "MISMATCH" not in r.stdout, r.stdout[-1500:]
