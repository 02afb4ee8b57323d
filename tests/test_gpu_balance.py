"""GPU parity for the colour balance (utils/color_correction/color_balance.cpp process_frame, modules/color_balance.py
balance) and the 8-bit HSV -> BGR conversion it uses, against the oracle's statement-by-statement restatement."""
import os
import subprocess
import sys

import numpy as np
import pytest

import balance_cases as BC
import frames as F

pytestmark = pytest.mark.gpu


def test_hsv2bgr_exhaustive(vp, oracle):
    """All 180 x 256 x 256 (h, s, v) triples plus the out-of-range hues 180..255: bit-exact with the oracle's vector form."""
    from vision.utils import color
    h, s, v = np.meshgrid(np.arange(256), np.arange(256), np.arange(256), indexing="ij")
    hsv = np.stack([h, s, v], -1).astype(np.uint8).reshape(256, 65536, 3)
    got, planes = color.hsv_to_bgr(hsv)
    exp = oracle.hsv2bgr(hsv, 0)
    assert np.array_equal(got, exp)
    assert all(np.array_equal(planes[c], got[:, :, c]) for c in range(3))
    # primaries (SURVEY A2 known answers, inverted)
    px = np.array([[[0, 255, 255], [60, 255, 255], [120, 255, 255], [0, 0, 255], [0, 0, 0], [15, 76, 200]]], np.uint8)
    assert color.hsv_to_bgr(px)[0].reshape(-1, 3).tolist() == [[0, 0, 255], [0, 255, 0], [255, 0, 0], [255, 255, 255], [0, 0, 0], [140, 170, 200]]


FLAG_SETS = [
    dict(),                                                                     # the reference's default call
    dict(hsv_contrast_correct=False),
    dict(equalize_rgb=False),
    dict(rgb_extrema_clipping=False),
    dict(rgb_contrast_correct=True),
    dict(rgb_contrast_correct=True, hsv_contrast_correct=False, rgb_extrema_clipping=False),
    dict(equalize_rgb=False, hsv_contrast_correct=False, rgb_extrema_clipping=False),   # identity
]


@pytest.mark.parametrize("flags", FLAG_SETS)
def test_balance_vs_oracle(vp, oracle, flags):
    from vision.modules.color_balance import balance
    for i, (w, h) in enumerate([(320, 180), (257, 101), (64, 64), (5, 3)]):
        for f in (F.s1_buoy(i, w, h), F.s2_bins(i, w, h), F.s3_noise(i, w, h)):
            got = balance(f, **flags)
            exp = oracle.color_balance(f, mean_mode=0, **flags)     # the reference's running tile mean (cpp:452-467), literally
            assert got.shape == f.shape and got.dtype == np.uint8
            assert np.array_equal(got, exp), (flags, w, h, int((got != exp).sum()))


def test_balance_flat_and_degenerate_frames(vp, oracle):
    """Frames where the reference's ranges collapse (all-equal channels): same output as the oracle's documented choices."""
    from vision.modules.color_balance import balance
    for val in (0, 7, 128, 255):
        f = np.full((40, 60, 3), val, np.uint8)
        assert np.array_equal(balance(f), oracle.color_balance(f, mean_mode=0))
    f = np.zeros((32, 32, 3), np.uint8)
    f[:, :, 2] = 200                                            # pure red: G and B means are 0 -> infinite gains
    assert np.array_equal(balance(f), oracle.color_balance(f, mean_mode=0))
    assert np.array_equal(balance(f, rgb_contrast_correct=True), oracle.color_balance(f, mean_mode=0, rgb_contrast_correct=True))


def test_balance_tiles(vp, oracle):
    from vision.modules.color_balance import balance
    f = F.s1_buoy(3, 320, 180)
    f[:90, :160] = (f[:90, :160] * 0.5).astype(np.uint8)        # one quadrant with a different cast
    for hb, vb in [(2, 2), (4, 3), (1, 5), (8, 1)]:
        for extra in (dict(), dict(hsv_contrast_correct=False)):
            got = balance(f, horizontal_blocks=hb, vertical_blocks=vb, **extra)
            exp = oracle.color_balance(f, horizontal_blocks=hb, vertical_blocks=vb, mean_mode=0, **extra)
            assert np.array_equal(got, exp), (hb, vb, extra)
    with pytest.raises(vp.VpError):
        balance(f, horizontal_blocks=3, vertical_blocks=1)      # 320 % 3 != 0: the reference wraps rows there


def test_balance_adaptive_cast_exact(vp, oracle):
    """adaptive_cast_correction (cpp:489-490) goes through pow((255. - v) / 255., 0.25): 256 possible arguments, tabulated with the
    host's libm (the one the reference would call here), so the result is exact, not within one."""
    from vision.modules.color_balance import balance
    for i, (w, h) in enumerate([(320, 180), (257, 101), (64, 64)]):
        for f in (F.s1_buoy(i, w, h), F.s2_bins(i, w, h), F.s3_noise(i, w, h)):
            for kw in (dict(hsv_contrast_correct=False), dict(), dict(rgb_contrast_correct=True)):
                got = balance(f, adaptive_cast_correction=True, **kw)
                exp = oracle.color_balance(f, adaptive_cast_correction=True, mean_mode=0, **kw)
                assert np.array_equal(got, exp), (w, h, kw, int((got != exp).sum()))


def test_balance_full_size_and_batch(vp, oracle):
    """1080p against the oracle, and the batched device entry against the single-frame entry."""
    import ctypes as C
    from vision import _vp
    from vision.modules.color_balance import balance
    f = F.s1_buoy(0)
    assert np.array_equal(balance(f), oracle.color_balance(f, mean_mode=0))
    n, h, w = 5, 72, 128
    frames = np.stack([F.s1_buoy(i, w, h) if i % 2 else F.s2_bins(i, w, h) for i in range(n)])
    ctx = _vp.default_context()
    L = _vp.lib()
    d = C.c_void_p()
    _vp.check(L.vp_dev_alloc(ctx.handle, frames.nbytes, C.byref(d)), ctx.handle)
    _vp.check(L.vp_memcpy_h2d(ctx.handle, d, _vp.ptr(frames), frames.nbytes), ctx.handle)
    _vp.check(L.vp_color_balance_dev(ctx.handle, d, d, w, h, n, _vp.CB_DEFAULT, 1, 1), ctx.handle)   # in place
    ctx.synchronize()
    out = np.empty_like(frames)
    _vp.check(L.vp_memcpy_d2h(ctx.handle, _vp.ptr(out), d, frames.nbytes), ctx.handle)
    _vp.check(L.vp_dev_free(ctx.handle, d), ctx.handle)
    for i in range(n):
        assert np.array_equal(out[i], balance(frames[i])), i


@pytest.mark.parametrize("flags", [dict(hsi_contrast_correct=True, hsv_contrast_correct=False), dict(hsi_contrast_correct=True),
                                   dict(hsi_contrast_correct=True, hsv_contrast_correct=False, equalize_rgb=False, rgb_extrema_clipping=False)])
def test_balance_hsi_stage_within_one(vp, oracle, flags):
    """hsi_contrast_correct (cpp:678-775): acos / cos come from the device libm, the oracle's from glibc; a last-bit difference
    can move a value across an integer before the truncating cast, so the tolerance is 1 on a small fraction of pixels.
    The order statistics (device radix select vs a sort) are exact, so nothing larger can appear."""
    from vision.modules.color_balance import balance
    for i, (w, h) in enumerate([(320, 180), (257, 101), (33, 7)]):
        for f in (F.s1_buoy(i, w, h), F.s2_bins(i, w, h), F.s3_noise(i, w, h)):
            got = balance(f, **flags)
            exp = oracle.color_balance(f, mean_mode=0, **flags)
            d = np.abs(got.astype(int) - exp.astype(int))
            assert d.max() <= 1, (flags, w, h, int(d.max()))
            assert (d > 0).mean() < 5e-3, (flags, w, h, float((d > 0).mean()))
    g = np.repeat(np.arange(0, 250, 1, dtype=np.uint8)[None, :, None], 40, 0).repeat(3, 2)
    assert np.array_equal(balance(g, equalize_rgb=False, hsv_contrast_correct=False, rgb_extrema_clipping=False, hsi_contrast_correct=True),
                          oracle.color_balance(g, equalize_rgb=False, hsv_contrast_correct=False, rgb_extrema_clipping=False, hsi_contrast_correct=True))
    flat = np.full((16, 16, 3), 90, np.uint8)
    assert np.array_equal(balance(flat, hsi_contrast_correct=True, hsv_contrast_correct=False),
                          oracle.color_balance(flat, hsi_contrast_correct=True, hsv_contrast_correct=False))


def _folds(vp):
    import ctypes as C
    ctx = vp.default_context()
    n = C.c_int32(-1)
    vp.check(vp.lib().vp_color_balance_last_folds(ctx.handle, C.byref(n)), ctx.handle)
    return n.value


def test_running_mean_is_reproduced_not_approximated(vp, oracle):
    """The reference's tile mean is a sequential fold (avg += (x - avg) / count, cpp:466-468).  The kernels build the gain tables
    from the exact mean only after checking that no value within a rigorous bound of it could change a table entry or a decision;
    otherwise they run the fold.  Both routes must give the reference's result (oracle mean_mode=0) - here on frames made to need
    the fold; with the fold forced for every tile (every tiling of balance_cases, and batches) in
    test_fold_forced_in_a_fresh_process, since libvp reads VP_CB_FORCE_FOLD once per process."""
    from vision.modules.color_balance import balance
    rng = np.random.default_rng(7)
    # 1. ordinary frames take the certified route: no tile folded
    f = F.s1_buoy(2, 320, 180)
    assert np.array_equal(balance(f), oracle.color_balance(f, mean_mode=0)) and _folds(vp) == 0
    assert np.array_equal(balance(f, horizontal_blocks=4, vertical_blocks=3), oracle.color_balance(f, horizontal_blocks=4, vertical_blocks=3, mean_mode=0))
    assert _folds(vp) == 0
    # 2. grey frames (B = G = R everywhere: one sequence, one fold value, gains exactly 1): certified as well
    g = np.repeat(rng.integers(0, 256, (90, 160, 1), dtype=np.uint8), 3, axis=2)
    assert np.array_equal(balance(g), oracle.color_balance(g, mean_mode=0)) and _folds(vp) == 0
    # 3. two channels with the same histogram but different sequences: exact means equal, folds not -> the order of the two largest
    #    means is in doubt -> fold
    a = rng.integers(60, 200, (90, 160), dtype=np.uint8)
    b = a.copy().ravel(); rng.shuffle(b); b = b.reshape(a.shape)
    lowc = (a // 3).astype(np.uint8)
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        planes = [a, b, lowc]
        f = np.stack([planes[order[0]], planes[order[1]], planes[order[2]]], -1)
        for kw in (dict(hsv_contrast_correct=False, rgb_extrema_clipping=False), dict()):
            got = balance(f, **kw)
            assert _folds(vp) == 1, (order, kw)
            assert np.array_equal(got, oracle.color_balance(f, mean_mode=0, **kw)), (order, kw)
    # 4. a tile mean sitting exactly on the 1/6 boundary of cpp:474: global mean 120, tile means 100 and 140
    f = np.zeros((40, 80, 3), np.uint8)
    f[:, :40] = (100, 50, 25); f[:, 40:] = (140, 70, 35)
    got = balance(f, horizontal_blocks=2, vertical_blocks=1, hsv_contrast_correct=False, rgb_extrema_clipping=False)
    assert _folds(vp) >= 1
    assert np.array_equal(got, oracle.color_balance(f, horizontal_blocks=2, vertical_blocks=1, hsv_contrast_correct=False, rgb_extrema_clipping=False, mean_mode=0))


def test_process_frame_symbol_and_tilings_that_do_not_divide(vp, oracle, capfd):
    """libauv-color-balance.so's `process_frame` (the symbol modules/color_balance.py:12-17 binds, color_balance.hpp:9-14), in place on
    the caller's BGR frame.  Tilings that divide the frame equal the oracle's statement of cpp:442-560.  A tiling that does NOT divide
    it is REJECTED by the kernels and balanced with one tile by the shim, with one line on stderr: the reference there grows the block
    count and lets the last column of tiles run on into the next image row (cpp:442-451, :461-464), so pixels are balanced twice, the
    second time from means taken over already-balanced pixels - an artefact of its indexing that no caller can want reproduced."""
    import ctypes as C
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = C.CDLL(os.path.join(root, "cuauv-vision-pipeline_amd", "lib", "libauv-color-balance.so"))
    lib.process_frame.restype = C.c_int
    lib.process_frame.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t] + [C.c_bool] * 6 + [C.c_int, C.c_int]

    def run(img, hb, vb):
        a = np.ascontiguousarray(img.copy())
        rc = lib.process_frame(a.ctypes.data, a.shape[0], a.shape[1], 3, True, False, True, False, True, False, hb, vb)   # (height, width, depth)
        return rc, a
    f = F.s1_buoy(5, 320, 180)
    f[:90, :160] = (f[:90, :160] * 0.6).astype(np.uint8)
    for hb, vb in [(1, 1), (2, 2), (4, 3)]:
        rc, got = run(f, hb, vb)
        assert rc == 0 and np.array_equal(got, oracle.color_balance(f, horizontal_blocks=hb, vertical_blocks=vb, mean_mode=0)), (hb, vb)
    capfd.readouterr()
    rc, got = run(f, 3, 1)                                     # 320 % 3 != 0
    err = capfd.readouterr().err
    assert np.array_equal(got, oracle.color_balance(f, horizontal_blocks=1, vertical_blocks=1, mean_mode=0))
    assert "do not divide" in err
    rc2, got2 = run(f, 3, 7)                                   # neither divides: same decision, reported once per kind of failure
    assert np.array_equal(got2, got)


HSI_FLAG_SETS = [dict(hsi_contrast_correct=True, hsv_contrast_correct=False), dict(hsi_contrast_correct=True),
                 dict(hsi_contrast_correct=True, hsv_contrast_correct=False, equalize_rgb=False, rgb_extrema_clipping=False)]   # as test_balance_hsi_stage_within_one


def test_tiles_keep_their_own_means(vp, oracle):
    """Frames whose tiles each have their own cast, inside the 1/6 band of cpp:474, so that every tile's own means reach its table
    (tests/test_balance_cases.py proves that from the oracle alone): a wrong tile lookup, table offset or per-tile histogram offset
    changes bytes.  Tile widths, frame widths and pixel counts that are no multiple of 4: the four-pixel groups of the three passes
    straddle tile edges and row ends, and the tail pixels run in the tiled kernels."""
    from vision.modules.color_balance import balance
    for name, f, hb, vb in BC.tiled_cases():
        for kw in (dict(), dict(hsv_contrast_correct=False), dict(rgb_contrast_correct=True), dict(adaptive_cast_correction=True)):
            got = balance(f, horizontal_blocks=hb, vertical_blocks=vb, **kw)
            BC.assert_exact(got, oracle.color_balance(f, horizontal_blocks=hb, vertical_blocks=vb, mean_mode=0, **kw), (name, kw))
        # without equalize_rgb the tiling is never read (cpp:441): one that does not divide the frame is taken as 1 x 1
        nhb, nvb = BC.NOT_DIVIDING[f.shape[:2]]
        assert f.shape[1] % nhb and f.shape[0] % nvb
        for kw in (dict(equalize_rgb=False), dict(equalize_rgb=False, rgb_contrast_correct=True)):
            got = balance(f, horizontal_blocks=nhb, vertical_blocks=nvb, **kw)
            BC.assert_exact(got, oracle.color_balance(f, mean_mode=0, **kw), (name, nhb, nvb, kw))


def test_small_frames(vp, oracle):
    """Frames of 1, 7 and 4 pixels: no full four-pixel group (or one group and a tail), ranges that collapse, percentile bounds of 0.
    The oracle returns a result for every non-HSI flag set at each of these sizes (tests/test_balance_cases.py checks it), so none is
    left out."""
    from vision.modules.color_balance import balance
    for i, (h, w) in enumerate(BC.SMALL_FRAMES):
        for f in (F.s1_buoy(i, w, h), F.s3_noise(i, w, h), F.s3_noise(10 + i, w, h) // 2 + 60):
            for flags in FLAG_SETS:
                BC.assert_exact(balance(f, **flags), oracle.color_balance(f, mean_mode=0, **flags), (h, w, flags))


@pytest.mark.parametrize("hb,vb", BC.BATCH_TILINGS)
def test_batch_every_stage_against_the_oracle(vp, oracle, hb, vb):
    """vp_color_balance_dev with n = 3 different frames, every stage, tiled and not, to a second buffer and in place: every frame
    against the oracle directly (the per-frame offsets into the histograms, tables, plans and HSI state), the source unchanged when
    it is not the destination, and nothing written past the destination."""
    frames = BC.batch_frames()
    exact = FLAG_SETS + [dict(adaptive_cast_correction=True)]
    for flags in exact + HSI_FLAG_SETS:
        exp = [oracle.color_balance(f, horizontal_blocks=hb, vertical_blocks=vb, mean_mode=0, **flags) for f in frames]
        for in_place in (False, True):
            rc, got, back, guard = BC.run_dev(vp, frames, BC.flag_bits(vp, **flags), hb, vb, in_place)
            assert rc == vp.OK, (flags, in_place, rc)
            for k in range(len(frames)):
                if flags in exact:
                    BC.assert_exact(got[k], exp[k], (flags, hb, vb, in_place, k))
                else:
                    BC.assert_hsi(got[k], exp[k], (flags, hb, vb, in_place, k))
            if not in_place:
                assert np.array_equal(back, frames), (flags, "the source was written")
            assert (guard == BC.FILL).all(), (flags, in_place, "bytes after the destination were written")


def test_tile_limit_and_refusals_through_the_c_abi(vp, oracle):
    """1024 tiles (one-pixel tiles: a tile count of 1 per histogram) are accepted, 1025 refused; batched frames that do not start
    4-byte aligned and, with equalize_rgb, a tiling that does not divide the frame are refused; a refusal writes nothing."""
    from vision.modules.color_balance import balance
    for (h, w), (hb, vb) in [((32, 32), (32, 32)), ((16, 64), (64, 16))]:
        f = BC.tiled_frame(h, w, hb, vb, 7)
        exp = oracle.color_balance(f, horizontal_blocks=hb, vertical_blocks=vb, mean_mode=0)
        assert not np.array_equal(exp, oracle.color_balance(f, mean_mode=0))        # the tiles' own means matter here too
        for in_place in (False, True):
            rc, got, back, guard = BC.run_dev(vp, f[None], vp.CB_DEFAULT, hb, vb, in_place)
            assert rc == vp.OK, (h, w, rc)
            BC.assert_exact(got[0], exp, (h, w, hb, vb, in_place))
            assert (guard == BC.FILL).all()
        BC.assert_exact(balance(f, horizontal_blocks=hb, vertical_blocks=vb), exp, (h, w, "host entry"))
    refused = [
        (BC.tiled_frame(25, 41, 1, 1, 8)[None], 41, 25),                                            # 1025 tiles
        (np.stack([F.s3_noise(0, 5, 3), F.s3_noise(1, 5, 3)]), 1, 1),                                # 45-byte frames in a batch
        (F.s1_buoy(0, 32, 32)[None], 3, 1),                                                          # 32 % 3 != 0 with equalize_rgb
    ]
    for frames, hb, vb in refused:
        rc, got, back, guard = BC.run_dev(vp, frames, vp.CB_DEFAULT, hb, vb, False)
        assert rc == vp.ERR_UNSUPPORTED, (frames.shape, hb, vb, rc)
        assert (got == BC.FILL).all() and (guard == BC.FILL).all(), (frames.shape, hb, vb, "a refused call wrote to the destination")
        assert np.array_equal(back, frames)
    with pytest.raises(vp.VpError):
        balance(BC.tiled_frame(25, 41, 1, 1, 8), horizontal_blocks=41, vertical_blocks=25)


def test_fold_forced_in_a_fresh_process():
    """VP_CB_FORCE_FOLD=1 makes k_cb_plan1 run the reference's sequential fold for every tile; libvp reads it once per process, so a
    fresh child runs every tiling of balance_cases and the batch of three against the oracle, checks after each call that every tile
    of every frame was folded, and exits non-zero at the first mismatch."""
    env = dict(os.environ)
    env["VP_CB_FORCE_FOLD"] = "1"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "_balance_fold_worker.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    assert "DONE 23" in r.stdout and "MISMATCH" not in r.stdout, r.stdout[-1500:]
