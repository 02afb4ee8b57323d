"""Bit-plane morphology over its dispatch space: which kernel runs (csrc/vp_morph.hip, planned by csrc/vp_morph_plan.h) is decided by
the frame's width and height and by the plan, so the shapes here are the last width on each side of every switch of the plan table
(tests/golden/morph_plan.txt, read by tests/morph_cases.py), the widths around one lap of 32 words (2048, 2049, 2112), 3840 and 8192,
at heights whose last 32- or 64-row strip has one row.  Everything is bit-exact against the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

import morph_cases as MC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ids(cases):
    return ["%s-%d" % c for c in cases]


_SINGLE = [(name, w) for name in MC.SINGLE_OPS for w in MC.widths_for(name)]
_PAIRS = [(name, w) for name in MC.CHAIN_PAIRS for w in MC.widths_for(name)]
_GENERAL_WIDTHS = sorted(set(MC.COMMON_WIDTHS) | set(MC.all_switch_widths()))


@pytest.mark.parametrize("name,w", _SINGLE, ids=_ids(_SINGLE))
def test_single_ops_at_the_specialised_shapes(vp, oracle, name, w):
    """erode, dilate, OPEN and CLOSE 3x3 and 5x5: eight of the twelve instantiations, with 64- and 32-row strips, one and several
    laps over the words of a row, and past the width at which the runtime-plan kernel takes over; on a host mask (the flag comes
    back) and on a device mask known to be 0/255 (binary_hint = 1)."""
    op, k = MC.SINGLE_OPS[name]
    for h in MC.HEIGHTS:
        for mname, m in MC.masks(h, w):
            MC.check_single(oracle, m, op, k, k, what=(name, mname))


@pytest.mark.parametrize("name,w", _PAIRS, ids=_ids(_PAIRS))
def test_open_close_pairs_through_the_chain(vp, oracle, name, w):
    """OPEN+CLOSE and CLOSE+OPEN (three merged stages: the other four instantiations) exist only through the chain: a batch of three
    different masks per shape, so that the block-to-(frame, strip) mapping meets a partial last strip in every frame."""
    for i, h in enumerate(MC.HEIGHTS):
        MC.check_chain(oracle, MC.chain_batch(h, w, first=(2 * i) % 5), MC.CHAIN_PAIRS[name], 1, "cleaned", what=name)


@pytest.mark.parametrize("w", _GENERAL_WIDTHS)
def test_plans_no_specialised_kernel_takes(vp, oracle, w):
    """7x7, 4x2 (the anchor off the centre: extents 2 | 1 and 1 | 0), 9x3 and 3x3 with three iterations at the same widths: the
    runtime-plan kernel's laps and its epilogue."""
    for _, op, (kw, kh), it in MC.GENERAL_OPS:
        for h in MC.HEIGHTS:
            for mname, m in MC.masks(h, w):
                MC.check_single(oracle, m, op, kw, kh, iterations=it, device=False, what=mname)


def _blocky(seed, h, w):
    """solid cells of 16 px with a sprinkling of single pixels and holes: something survives an OPEN 21x21"""
    rng = np.random.default_rng(seed)
    m = np.kron((rng.random(((h + 15) // 16, (w + 15) // 16)) < 0.7).astype(np.uint8) * 255, np.ones((16, 16), np.uint8))[:h, :w]
    m = np.ascontiguousarray(m)
    m[rng.random((h, w)) < 0.004] ^= 255
    return m


@pytest.mark.parametrize("name,op", [("close71x71", MC.CLOSE), ("open71x71", MC.OPEN)])
def test_two_launches(vp, oracle, name, op):
    """71x71 at 70 x 3840: four stages (31 + 4 per kind) whose halo of 140 rows takes two launches through the scratch plane"""
    assert MC.plan_case(name, 70, 3840)["launches"] == 2
    for mname, m in MC.masks(70, 3840) + [("blocky", _blocky(5, 70, 3840))]:
        MC.check_single(oracle, m, op, 71, 71, what=(name, mname))


@pytest.mark.parametrize("ccl,source", [(2, "threshed"), (1, "cleaned")])
def test_three_launches_leave_the_threshold_plane_alone(vp, oracle, ccl, source):
    """Eight alternating OPEN / CLOSE 21x21 at 40 x 3840: nine stages with a halo of 320 rows against 128 per launch.  From the third
    launch on, run_bit_stages used to swap its input plane - the chain's threshold bits - into the ping-pong, and the second launch
    overwrote what ccl = 2 and contours of `threshed` read afterwards; the plan never makes the input a destination now."""
    case = MC.plan_case("chain8x21", 40, 3840)
    assert case["launches"] >= 3 and not any(p.endswith(">0") for p in case["planes"].split(","))
    morph = [(MC.CLOSE if i % 2 else MC.OPEN, 21, 21, 1) for i in range(8)]
    MC.check_chain(oracle, [_blocky(11, 40, 3840), _blocky(12, 40, 3840)], morph, ccl, source, what="chain8x21")


def test_too_wide_for_the_strip_is_refused_cleanly(vp, oracle):
    """erode 5x45 on a 0/255 mask of 40 x 8192: 32 + 44 rows of 128 words, twice, exceed the LDS budget of one launch.  The call is
    refused (VP_ERR_UNSUPPORTED) before anything is written, the context goes on working, and grey-level input of the same size
    takes the generic kernel as before."""
    from vision.utils import transform as T
    assert MC.plan_case("erode5x45", 40, 8192) == "refused"
    m = dict(MC.masks(40, 8192))["p0.9"]
    k = np.ones((45, 5), np.uint8)
    with pytest.raises(vp.VpError, match="unsupported|too wide"):
        np.asarray(T.erode(m, k))            # (a deferred result launches when it is first looked at)
    L, ctx = vp.lib(), vp.default_context()
    src = np.ascontiguousarray(m)
    dst = np.full_like(src, 0xA5)
    rc = L.vp_morph_u8(ctx.handle, vp.MORPH_ERODE, vp.ptr(src), 8192, 40, 1, vp.ptr(k), 5, 45, -1, -1, 1, vp.ptr(dst))
    assert rc == vp.ERR_UNSUPPORTED and b"too wide" in L.vp_last_error(ctx.handle)
    assert (dst == 0xA5).all(), "a refused call wrote to its destination"
    k5 = np.ones((5, 5), np.uint8)
    assert np.array_equal(np.asarray(T.erode(m, k5)), oracle.morph(oracle.ERODE, m, k5, fast=True))
    g = np.random.default_rng(3).integers(0, 256, (40, 8192), dtype=np.uint8)
    assert np.array_equal(np.asarray(T.erode(g, k)), oracle.morph(oracle.ERODE, g, k))


@pytest.mark.parametrize("switch", ["VP_NO_SYM", "VP_MORPH_STRIP32"])
def test_fallback_kernels_on_the_common_shapes(switch):
    """The runtime-plan kernel (VP_NO_SYM=1) and the 32-row instantiations (VP_MORPH_STRIP32=1) on shapes where the 64-row specialised
    kernels normally win.  libvp reads both once per process: a fresh child runs the cases and exits non-zero at the first mismatch."""
    env = {k: v for k, v in os.environ.items() if k not in ("VP_NO_SYM", "VP_MORPH_STRIP32")}
    env[switch] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_morph_fallback_worker.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    assert "DONE 36" in r.stdout and "MISMATCH" not in r.stdout, r.stdout[-1500:]
