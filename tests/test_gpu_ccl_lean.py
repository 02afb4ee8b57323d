"""What the two-level labelling queues behind its merge: the six launches of the crowded-frame kernels (FULL) or one launch that
finishes a handed-over frame slowly (LEAN), chosen by a hint from an earlier call (VP_OPT_CCL_CROWDED, csrc/vp_ccl_hint.h).  Both must
give cv2's result: every output here - labels, stats, centroids, nlabels - is compared bitwise with the oracle's, in both numberings,
with either form forced and in automatic mode, where the number of launches the call queued tells which form ran
(with labels: local, merge, stand-in, write = 4 in LEAN; local, merge, six crowded-frame launches, write = 9 in FULL)."""
import numpy as np
import pytest

import ccl_cases as CC
import frames as F

pytestmark = pytest.mark.gpu

AUTO, FULL, LEAN = 0, 1, 2
SIZES = [(65, 33), (257, 97), (640, 200)]          # (w, h)
DENSITIES = [0.02, 0.1, 0.5]

_CACHE = {}


def _mask(w, h, p):
    key = ("mask", w, h, p)
    if key not in _CACHE:
        _CACHE[key] = F.random_mask(np.random.default_rng(w * 1000 + h + int(p * 100)), h, w, p)
    return _CACHE[key]


def _ref(oracle, m, numbering):
    key = ("ref", m.shape, hash(m.tobytes()), numbering)
    if key not in _CACHE:
        _CACHE[key] = oracle.ccl(m, block=numbering)
    return _CACHE[key]


_segments = CC.segments


def _crowded_strip(oracle, m):
    """True when some strip of the strip-local pass holds more than rc components or more than cap2 word segments (what hands a frame
    over); strip height and cap2 are the frame's own (ccl_cases.geom, ccl_cases.cap2)."""
    h, w = m.shape
    rows, cap2 = CC.geom(h, w)[0], CC.cap2(h, w)
    for y in range(0, h, rows):
        part = np.ascontiguousarray(m[y:y + rows])
        if oracle.ccl(part, block=2)[0] - 1 > CC.RC or _segments(part) > cap2:
            return True
    return False


def _ccl(vp, ctx, m, numbering, max_labels, want_labels=True):
    h, w = m.shape
    labels = np.empty((h, w), np.int32) if want_labels else None
    stats = np.empty((max_labels, 5), np.int32)
    cent = np.empty((max_labels, 2), np.float64)
    n = vp.C.c_int32(0)
    vp.check(vp.lib().vp_ccl_u8(ctx.handle, vp.ptr(m), m.strides[0], w, h, int(numbering), vp.ptr(labels), vp.ptr(stats), vp.ptr(cent),
                                int(max_labels), vp.C.byref(n)), ctx.handle)
    return n.value, labels, stats, cent


def _check_one(vp, ctx, oracle, m, numbering, max_labels=None, want_labels=True):
    ml = m.size + 2 if max_labels is None else max_labels
    n, lab, st, ce = _ccl(vp, ctx, m, numbering, ml, want_labels)
    on, olab, ost, oce = _ref(oracle, m, numbering)
    assert n == on
    if want_labels:
        assert np.array_equal(lab, olab)
    k = min(on, ml)
    assert np.array_equal(st[:k], ost[:k])
    assert np.array_equal(ce[:k].view(np.uint64), oce[:k].view(np.uint64))       # bitwise, NaN included
    assert not st[k:].any() and not ce[k:].view(np.uint64).any()                 # rows past the last label: zeros (the buffers came from np.empty)


@pytest.fixture
def forced(vp, request):
    ctx = vp.default_context()
    ctx.set_option(vp.OPT_CCL_CROWDED, request.param)
    yield ctx, request.param
    ctx.synchronize()
    ctx.set_option(vp.OPT_CCL_CROWDED, AUTO)


def _launches(mode, labels=True):
    return (4 if mode == LEAN else 9) - (0 if labels else 1)


@pytest.mark.parametrize("forced", [LEAN, FULL], indirect=True, ids=["lean", "full"])
@pytest.mark.parametrize("numbering", [2, 1])
@pytest.mark.parametrize("w,h", SIZES)
def test_noise_frames(vp, oracle, forced, numbering, w, h):
    ctx, mode = forced
    for p in DENSITIES:
        m = _mask(w, h, p)
        if (w, h) != SIZES[0]:
            assert _crowded_strip(oracle, m), (w, h, p)
        elif p == DENSITIES[0]:
            assert not _crowded_strip(oracle, m) and _segments(m[:32]) <= CC.cap2(h, w) == 32 * 2 + 2      # not handed over: resolved by the merge
        _check_one(vp, ctx, oracle, m, numbering)
        assert ctx.ccl_last_launches() == _launches(mode)
        _check_one(vp, ctx, oracle, m, numbering, want_labels=False)                      # statistics only
        assert ctx.ccl_last_launches() == _launches(mode, labels=False)


@pytest.mark.parametrize("forced", [LEAN, FULL], indirect=True, ids=["lean", "full"])
def test_fewer_labels_than_components(vp, oracle, forced):
    ctx, _ = forced
    m = _mask(257, 97, 0.1)
    assert _ref(oracle, m, 2)[0] > 200
    for numbering in (2, 1):
        _check_one(vp, ctx, oracle, m, numbering, max_labels=37)
        _check_one(vp, ctx, oracle, m, numbering, max_labels=1, want_labels=False)


def _gray_frames(masks):
    return np.repeat(np.stack(masks)[..., None], 3, axis=3)


@pytest.mark.parametrize("forced", [LEAN, FULL], indirect=True, ids=["lean", "full"])
@pytest.mark.parametrize("crowded_at", [0, 3], ids=["crowded first", "crowded last"])
def test_mixed_batch(vp, oracle, forced, crowded_at):
    """A batch of four: blobs, flat zero, all foreground and one crowded frame, the crowded one first or last; with and without the
    label image."""
    from vision.utils import chain
    w, h = 257, 97
    yy, xx = np.mgrid[0:h, 0:w]
    blobs = np.zeros((h, w), np.uint8)
    rng = np.random.default_rng(7)
    for _ in range(6):
        cx, cy, r = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(4, 25)
        blobs[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 255
    masks = [blobs, np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)]
    masks.insert(crowded_at, _mask(w, h, 0.1))
    ml = w * h + 2
    for numbering in (vp.CCL_BLOCK2X2, vp.CCL_PIXEL):
        for want in (("threshed", "labels", "stats"), ("stats",)):
            out = chain.run_chain(_gray_frames(masks), vp.BGR2GRAY, (128, 0, 0), (255, 255, 255), [], ccl=1, numbering=numbering, max_labels=ml, want=want)
            for f, m in enumerate(masks):
                on, olab, ost, oce = _ref(oracle, m, numbering)
                if "threshed" in want:
                    assert np.array_equal(out["threshed"][f], m), f
                    assert np.array_equal(out["labels"][f], olab), f
                assert int(out["nlabels"][f]) == on, f
                assert np.array_equal(out["stats"][f][:on], ost), f
                assert np.array_equal(out["centroids"][f][:on].view(np.uint64), oce.view(np.uint64)), f
                assert not out["stats"][f][on:].any(), f


def test_automatic_mode_follows_the_hint(vp, oracle):
    """One context of its own: clean x 2, crowded x 3, clean x 34.  Every call's outputs equal the oracle's; the launch counts show the
    mode: LEAN until the hint of the first crowded call is read (crowded 2), FULL until the 32nd quiet hint in a row is read - the
    hint of clean 3 is read by clean 4, so that is clean 35.  vp_ccl_u8 returns results to the host, so every hint is fresh."""
    ctx = vp.Context(0)
    try:
        clean, crowded = _mask(65, 33, 0.02), _mask(257, 97, 0.1)
        seq = [(clean, 4)] * 2 + [(crowded, 4)] + [(crowded, 9)] * 2 + [(clean, 9)] * 32 + [(clean, 4)] * 2
        assert len(seq) == 39
        for i, (m, want) in enumerate(seq):
            _check_one(vp, ctx, oracle, m, 2)
            assert ctx.ccl_last_launches() == want, (i, ctx.ccl_last_launches(), want)
    finally:
        ctx.close()


def test_1080p_frame_forced_lean(vp, oracle):
    """The plan of the workload's size (34 strips of 32 rows, 30 words per row): one frame of 10 % noise through the stand-in launch."""
    ctx = vp.default_context()
    fr = F.s3_noise(0)
    m = oracle.inrange(oracle.bgr2gray(fr), 190, 255)                  # 10 % of the pixels (the grey of uniform noise is bell-shaped)
    assert 0.08 < (m > 0).mean() < 0.13
    assert _crowded_strip(oracle, m)
    ctx.set_option(vp.OPT_CCL_CROWDED, LEAN)
    try:
        _check_one(vp, ctx, oracle, m, 2, max_labels=1 << 18)
        assert ctx.ccl_last_launches() == 4
    finally:
        ctx.synchronize()
        ctx.set_option(vp.OPT_CCL_CROWDED, AUTO)


def test_stream_switch_across_the_mode_switch(vp, oracle):
    """tests/test_gpu_ccl_levels.py's two-stream sequence in automatic mode on a context of its own: the first handed-over frame goes
    through the stand-in launch, the context moves to a second stream where the next one finds the crowded-frame kernels queued, and
    back.  Every call has finished before the stream changes."""
    import torch
    ctx = vp.Context(0)
    rng = np.random.default_rng(33 * 31 + 65)
    a, b = F.random_mask(rng, 33, 65, 0.5), F.random_mask(rng, 33, 65, 0.5)
    side = torch.cuda.Stream()
    ctx.set_option(vp.OPT_CCL_MERGE_CAP, 0)
    try:
        _check_one(vp, ctx, oracle, a, 2)
        assert ctx.ccl_last_launches() == 4
        ctx.synchronize()
        ctx.set_stream(side.cuda_stream)
        _check_one(vp, ctx, oracle, b, 2)
        assert ctx.ccl_last_launches() == 9
        ctx.synchronize()
        ctx.set_stream(None)
        _check_one(vp, ctx, oracle, a, 2)
        assert ctx.ccl_last_launches() == 9
    finally:
        ctx.synchronize()
        ctx.set_stream(None)
        ctx.close()
