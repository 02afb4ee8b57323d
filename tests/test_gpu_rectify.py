"""GPU suite for vp_rectify_pair_*: byte for byte against tests/rectify_restate.py over tests/rectify_cases.py (sizes that straddle the
tile of vp_rectify_pair_plan, rows of 1, 3, 4 and 5 pixels, 1, 3 and 4 channels, both, one and no colour result, tables that reach
every border rule), against the composition of the existing GPU entries (vp_remap_fixed_dev, then vp_cvt_color_dev), on padded
strides, on a side-by-side frame, and through the Python layer."""
import numpy as np
import pytest

import rectify_cases as RC
import rectify_restate as R

pytestmark = pytest.mark.gpu

PLAN = RC.plan()
CASES = RC.cases(PLAN["tile_w"], PLAN["tile_h"])


def _dev(vp, arr):
    from vision.devmat import DeviceMat
    return DeviceMat.from_host(vp.default_context(), arr)


def dev_rectify(vp, left, right, tl, tr, keep="both", spad=0, gpad=0, cpad=0):
    """vp_rectify_pair_dev on padded device images -> (grey left, grey right, colour left | None, colour right | None); the padding
    and the sources must come back untouched"""
    ctx = vp.default_context()
    cn = 1 if left.ndim == 2 else left.shape[2]
    h, w = left.shape[:2]
    oh, ow = tl[1].shape
    src = []
    for img in (left, right):
        buf = np.full((h, w * cn + spad), 0x5A, np.uint8)
        buf[:, :w * cn] = img.reshape(h, w * cn)
        src.append(buf)
    dsrc = [_dev(vp, b) for b in src]
    dt = [_dev(vp, a) for a in (tl[0], tl[1], tr[0], tr[1])]
    grey = [_dev(vp, np.full((oh, ow + gpad), 0xA5, np.uint8)) for _ in range(2)]
    col = [_dev(vp, np.full((oh, ow * cn + cpad), 0xA5, np.uint8)) if keep == "both" or (keep == "left" and e == 0) else None for e in range(2)]
    ptr = lambda m: None if m is None else m.dev_ptr
    vp.check(vp.lib().vp_rectify_pair_dev(ctx.handle, dsrc[0].dev_ptr, w * cn + spad, dsrc[1].dev_ptr, w * cn + spad, w, h, cn, dt[0].dev_ptr, dt[1].dev_ptr, dt[2].dev_ptr,
                                          dt[3].dev_ptr, ow, oh, grey[0].dev_ptr, ow + gpad, grey[1].dev_ptr, ow + gpad, ptr(col[0]), ow * cn + cpad, ptr(col[1]),
                                          ow * cn + cpad), ctx.handle)
    out = []
    for g in grey:
        host = g.host_copy()
        assert np.all(host[:, ow:] == 0xA5), "the padding of a grey result was written"
        out.append(np.ascontiguousarray(host[:, :ow]))
    for c in col:
        if c is None:
            out.append(None)
            continue
        host = c.host_copy()
        assert np.all(host[:, ow * cn:] == 0xA5), "the padding of a colour result was written"
        out.append(np.ascontiguousarray(host[:, :ow * cn]).reshape((oh, ow) if cn == 1 else (oh, ow, cn)))
    for d, b in zip(dsrc, src):
        assert np.array_equal(d.host_copy(), b), "a source was written"
    for d, a in zip(dt, (tl[0], tl[1], tr[0], tr[1])):
        assert np.array_equal(d.host_copy(), a), "a table was written"
    return out


def composed(vp, img, table):
    """the same eye from the existing entries: vp_remap_fixed_dev, then vp_cvt_color_dev on its result"""
    ctx = vp.default_context()
    from vision.devmat import DeviceMat
    cn = 1 if img.ndim == 2 else img.shape[2]
    h, w = img.shape[:2]
    oh, ow = table[1].shape
    src, xy, fr = _dev(vp, img), _dev(vp, table[0]), _dev(vp, table[1])
    col = DeviceMat(ctx, (oh, ow) if cn == 1 else (oh, ow, cn), np.uint8)
    zero = np.zeros(4, np.uint8)
    vp.check(vp.lib().vp_remap_fixed_dev(ctx.handle, src.dev_ptr, w * cn, w, h, cn, xy.dev_ptr, fr.dev_ptr, ow, oh, vp.INTER_LINEAR, vp.BORDER_CONSTANT, zero.ctypes.data,
                                         col.dev_ptr), ctx.handle)
    if cn == 1:
        return col.host_copy(), col.host_copy()
    grey = DeviceMat(ctx, (oh, ow), np.uint8)
    vp.check(vp.lib().vp_cvt_color_dev(ctx.handle, vp.BGR2GRAY if cn == 3 else vp.BGRA2GRAY, col.dev_ptr, ow * cn, ow, oh, grey.dev_ptr, None), ctx.handle)
    return grey.host_copy(), col.host_copy()


def _same(got, want, keep):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), f"{int((got[0] != want[0]).sum() + (got[1] != want[1]).sum())} grey pixels differ"
    assert (got[2] is None) == (keep == "none") and (got[3] is None) == (keep != "both")
    assert got[2] is None or np.array_equal(got[2], want[2]), "the left colour result differs"
    assert got[3] is None or np.array_equal(got[3], want[3]), "the right colour result differs"


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_every_entry_form_equals_the_statement(vp, case):
    left, right, tl, tr = RC.inputs(case)
    want = RC.expected(case)
    if case["table"] == "outside":
        assert not want[0].any() and not want[3].any()
    _same(dev_rectify(vp, left, right, tl, tr, case["keep"]), want, case["keep"])
    _same(dev_rectify(vp, left, right, tl, tr, case["keep"], spad=3, gpad=5, cpad=7), want, case["keep"])           # odd paddings: rows of every alignment
    _same(dev_rectify(vp, left, right, tl, tr, case["keep"], spad=4, gpad=8, cpad=16), want, case["keep"])          # rows that keep their alignment
    # host images and tables in and out
    ctx = vp.default_context()
    cn, oh, ow = case["cn"], case["oh"], case["ow"]
    grey = [np.empty((oh, ow), np.uint8) for _ in range(2)]
    col = [np.empty((oh, ow) if cn == 1 else (oh, ow, cn), np.uint8) if case["keep"] == "both" or (case["keep"] == "left" and e == 0) else None for e in range(2)]
    p = lambda a: None if a is None else a.ctypes.data
    vp.check(vp.lib().vp_rectify_pair_u8(ctx.handle, p(left), p(right), case["w"], case["h"], cn, p(tl[0]), p(tl[1]), p(tr[0]), p(tr[1]), ow, oh, p(grey[0]), p(grey[1]),
                                         p(col[0]), p(col[1])), ctx.handle)
    _same(grey + col, want, case["keep"])


@pytest.mark.parametrize("case", [c for c in CASES if c["keep"] == "both" and c["ow"] == 40], ids=lambda c: c["id"])
def test_equals_the_composition_of_the_existing_entries(vp, case):
    left, right, tl, tr = RC.inputs(case)
    got = dev_rectify(vp, left, right, tl, tr)
    for e, (img, t) in enumerate(((left, tl), (right, tr))):
        grey, col = composed(vp, img, t)
        assert np.array_equal(got[e], grey) and np.array_equal(got[2 + e], col)


def test_a_tap_beside_the_eye_is_the_border_not_the_neighbour(vp):
    """a side-by-side frame, left eye black, right eye white, and a left table that taps column w - 1 with a fraction: a gather that
    clamped against the stride would blend in the right eye's column 0"""
    ctx = vp.default_context()
    w, h = 260, 5
    frame = np.zeros((h, 2 * w, 3), np.uint8)
    frame[:, w:] = 255
    xy = np.zeros((h, w, 2), np.int16)
    xy[..., 0], xy[..., 1] = w - 1, np.arange(h)[:, None]
    frac = np.full((h, w), 7 * 32 + 19, np.uint16)
    ident = RC.table("identity", w, h, w, h, 0)
    dframe, dt = _dev(vp, frame), [_dev(vp, a) for a in (xy, frac, ident[0], ident[1])]
    grey = [_dev(vp, np.full((h, w), 9, np.uint8)) for _ in range(2)]
    vp.check(vp.lib().vp_rectify_pair_dev(ctx.handle, dframe.dev_ptr, 6 * w, dframe.dev_ptr + 3 * w, 6 * w, w, h, 3, dt[0].dev_ptr, dt[1].dev_ptr, dt[2].dev_ptr, dt[3].dev_ptr,
                                          w, h, grey[0].dev_ptr, w, grey[1].dev_ptr, w, None, 0, None, 0), ctx.handle)
    assert not grey[0].host_copy().any(), "the left eye read the right eye's pixels"
    assert np.all(grey[1].host_copy() == 255)


def _rig():
    from vision.utils import stereo
    K1 = np.array([[112.3, 0, 47.4], [0, 111.1, 31.9], [0, 0, 1.0]])
    K2 = np.array([[109.8, 0, 48.7], [0, 110.4, 30.2], [0, 0, 1.0]])
    return stereo.StereoRig(K1, [-0.28, 0.09, 0.0005, -0.0003, -0.013], K2, [-0.27, 0.08, -0.0004, 0.0006, -0.012], (96, 64), stereo.rodrigues([0.01, -0.02, 0.03]),
                            [-0.12, 0.004, -0.003])


def test_python_layer(vp):
    from vision.devmat import DeviceMat
    from vision.utils import stereo
    rig = _rig()
    w, h = rig.size
    assert rig.tables[0].shape == (h, w) and rig.focal_px == rig.P1[0, 0] and abs(rig.baseline_m - np.linalg.norm([-0.12, 0.004, -0.003])) < 1e-12
    tabs = [(t.xy.host_copy(), t.frac.host_copy()) for t in rig.tables]
    assert not np.array_equal(tabs[0][0], tabs[1][0])
    for cn in (1, 3, 4):
        frame = RC.image(h, 2 * w, cn, 5 + cn)
        left, right = np.ascontiguousarray(frame[:, :w]), np.ascontiguousarray(frame[:, w:])
        want = R.rectify_pair(left, right, *tabs)
        got = stereo.rectify_pair(left, right, *rig.tables, colour=True)
        assert len(got) == 4 and all(isinstance(g, np.ndarray) for g in got) and all(np.array_equal(g, x) for g, x in zip(got, want))
        got = stereo.rectify_pair(left, right, *rig.tables)
        assert len(got) == 2 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        dev = stereo.rectify_pair(_dev(vp, left), right, *rig.tables, colour=True)
        assert all(isinstance(g, DeviceMat) for g in dev) and all(np.array_equal(g.host_copy(), x) for g, x in zip(dev, want))
        assert np.array_equal(dev[2].host_copy(), rig.tables[0].apply(left)), "the colour result is the table's own remap"
        # a side-by-side frame is split by pointer
        halves = stereo.rectify_pair(_dev(vp, left), _dev(vp, right), *rig.tables, colour=True)
        dframe = _dev(vp, frame)
        whole = rig.rectify(dframe, colour=True)
        assert all(isinstance(g, DeviceMat) for g in whole) and all(np.array_equal(a.host_copy(), b.host_copy()) for a, b in zip(whole, halves))
        assert np.array_equal(dframe.host_copy(), frame)
        host = rig.rectify(frame)
        assert len(host) == 2 and isinstance(host[0], np.ndarray) and np.array_equal(host[0], want[0]) and np.array_equal(host[1], want[1])
        pair = rig.rectify(left, right)
        assert np.array_equal(pair[0], want[0]) and np.array_equal(pair[1], want[1])
    with pytest.raises(ValueError):
        rig.rectify(np.zeros((h, 2 * w + 2, 3), np.uint8))
    with pytest.raises(ValueError):
        rig.rectify(np.zeros((h, w, 2), np.uint8), np.zeros((h, w, 2), np.uint8))
    with pytest.raises(ValueError):
        stereo.rectify_pair(np.zeros((h, w, 3), np.uint8), np.zeros((h, w), np.uint8), *rig.tables)
