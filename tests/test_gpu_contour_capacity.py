"""The contour pass on the two sides of every head count and capacity it compares a count with: the six instantiations of the one-block
bookkeeping with its tables in LDS (k_ct_jump: ctj_body_lds<1|2|3|4|6|8>, the last head count of each and the first of the next), the
one-block form with the tables in global memory (8193 heads), the launches over the chip, the pass that is deferred and repeated, the
hierarchy at 127 .. 257 borders, and the caller's capacities met exactly, through the C ABI.  The masks come from tests/contour_cases.py,
whose head counts tests/test_contour_cases.py checks on the CPU; that a mask ran the form it was built for is read back from
vp_contours_last_heads.  Expected results: oracle.find_contours and tests/contour_tree_restate.py, nothing else."""
import ctypes as C

import numpy as np
import pytest

import contour_cases as CC
import contour_tree_restate as R

pytestmark = pytest.mark.gpu

CASES = CC.boundary_cases()
IDS = [c[0] for c in CASES]
FILL, HOLE_FILL, GUARD = -7, 7, 16
FORMS = [("one_block", "0"), ("launches", "1")]


@pytest.fixture(scope="module")
def ctx(vp):
    """A context of this file's own: no batched pass ever runs on it, so vp_contours_last_heads is the head count of its last
    single-image pass and nothing else."""
    c = vp.Context(0)
    yield c
    c.close()


_REF = {}


def _ref(oracle, key, m, mode, method):
    k = (key, mode, method)
    if k not in _REF:
        cs, holes = oracle.find_contours(m, mode, method, with_holes=True)
        _REF[k] = (tuple(cs), holes, sum(len(c) for c in cs))
    return _REF[k]


def _tree_ref(oracle, key, m, mode, method):
    k = (key, mode, method, "tree")
    if k not in _REF:
        _REF[k] = R.expected(m, mode, list(_ref(oracle, key, m, 1, method)[0]), R.raster_scan)
    return _REF[k]


def _call(vp, ctx, m, mode, method, max_c, max_p, entry="u8", tree=False):
    """one direct call of a C entry with arrays of exactly the capacities given plus GUARD elements behind each"""
    h, w = m.shape
    pts = np.full((max_p + GUARD, 2), FILL, np.int32)
    counts = np.full(max_c + GUARD, FILL, np.int32)
    holes = np.full(max_c + GUARD, HOLE_FILL, np.uint8)
    hier = np.full((max_c + GUARD, 4), FILL, np.int32) if tree else None
    nc, npts = C.c_int32(-1), C.c_int64(-1)
    args = [int(mode), int(method), vp.ptr(pts), int(max_p), vp.ptr(counts), vp.ptr(holes), int(max_c), C.byref(nc), C.byref(npts)]
    if tree:
        args.append(vp.ptr(hier))
    name = "vp_find_contours_" + ("tree_" if tree else "") + entry
    if entry == "u8":
        vp.check(getattr(vp.lib(), name)(ctx.handle, vp.ptr(m), m.strides[0], w, h, *args), ctx.handle)
    else:
        from vision.devmat import DeviceMat
        d = DeviceMat.from_host(ctx, np.ascontiguousarray(m), binary=True)
        vp.check(getattr(vp.lib(), name)(ctx.handle, d.dev_ptr, w, w, h, *args), ctx.handle)
    return nc.value, npts.value, pts, counts, holes, hier


def _lists(k, pts, counts):
    out, o = [], 0
    for c in counts[:k].tolist():
        out.append(pts[o:o + c].reshape(-1, 1, 2))
        o += c
    return out


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def _heads(vp, ctx):
    return int(vp.lib().vp_contours_last_heads(ctx.handle))


def _check_fit(vp, ctx, oracle, key, m, mode, method, entry="u8"):
    ec, eh, P = _ref(oracle, key, m, mode, method)
    k, p, pts, counts, holes, _ = _call(vp, ctx, m, mode, method, len(ec) + 3, P + 5, entry)
    assert (k, p) == (len(ec), P), (k, p, len(ec), P)
    assert _same(_lists(k, pts, counts), ec), "contours, their order or their start points"
    assert np.array_equal(holes[:k], eh), "hole flags"


@pytest.mark.parametrize("name,fam,H,shape", CASES, ids=IDS)
def test_head_count_is_the_restatement(vp, oracle, ctx, monkeypatch, name, fam, H, shape):
    """vp_contours_last_heads after a pass in the dense cut (VP_CT_MANY=0) and in the sparse one (VP_CT_MANY=1) against
    contour_cases.head_count: k_ct_headmaps and k_ct_prefix against the definition, and the proof that the case has the H it was built
    for when the bookkeeping picks its instantiation."""
    m = CC.build(fam, H, shape)
    monkeypatch.setenv("VP_CT_MANY", "0")
    _check_fit(vp, ctx, oracle, name, m, 1, 2)
    assert _heads(vp, ctx) == CC.head_count(m) == H
    monkeypatch.setenv("VP_CT_MANY", "1")
    _check_fit(vp, ctx, oracle, name, m, 1, 2)
    assert _heads(vp, ctx) == CC.head_count(m, sparse=True)


def test_head_count_of_random_masks(vp, oracle, ctx, monkeypatch):
    """200 masks of random 4x4 patterns edge to edge (every local shape, at sizes from one word to two and odd widths) and three noise
    masks: the head count in both cuts, and RETR_LIST against the oracle."""
    rng = np.random.default_rng(17)
    masks = [CC.tiled_4x4(rng, int(rng.integers(4, 25)), int(rng.integers(4, 100))) for _ in range(200)]
    masks += [(rng.random((64, 200)) < p).astype(np.uint8) * 255 for p in (0.3, 0.5, 0.7)]
    for i, m in enumerate(masks):
        for many in ("0", "1"):
            monkeypatch.setenv("VP_CT_MANY", many)
            ec, eh, P = _ref(oracle, ("random", i), m, 1, 2)
            k, p, pts, counts, holes, _ = _call(vp, ctx, m, 1, 2, len(ec) + 1, P + 1)
            assert (k, p) == (len(ec), P) and _same(_lists(k, pts, counts), ec) and np.array_equal(holes[:k], eh), (i, many)
            assert _heads(vp, ctx) == CC.head_count(m, sparse=many == "1"), (i, many, m.shape)


@pytest.mark.parametrize("name,fam,H,shape", CASES, ids=IDS)
def test_every_instantiation_boundary(vp, oracle, ctx, monkeypatch, name, fam, H, shape):
    """b and b + 1 heads for every b at which k_ct_jump changes the instantiation (and, past 8192, to the tables in global memory): both
    retrieval modes, both approximations, both entries - contours, points, order, start points and hole flags as the oracle's."""
    monkeypatch.setenv("VP_CT_MANY", "0")
    m = CC.build(fam, H, shape)
    for mode in (0, 1):
        for method in (1, 2):
            _check_fit(vp, ctx, oracle, name, m, mode, method, "u8" if method == 1 else "dev")
            assert _heads(vp, ctx) == H


@pytest.mark.parametrize("H", [CC.LDS_HEADS, CC.LDS_HEADS + 1])
@pytest.mark.parametrize("fam", CC.FAMILIES)
def test_three_routes_around_the_lds_capacity(vp, oracle, ctx, monkeypatch, fam, H):
    """8192 and 8193 heads with the form forced to one block (tables in LDS, then in global memory), forced to launches, and left to the
    context: after a small mask the call starts as one block, a frame of 8193 heads answers "too many" and the pass is repeated as
    launches inside the same call - whose head count is then the sparse cut's, the only trace the repeat leaves; 8192 is not repeated."""
    shape = CC.shape_for(CC.LDS_HEADS)
    m = CC.build(fam, H, shape)
    name = f"{fam}-{H}"
    sparse = CC.head_count(m, sparse=True)
    assert sparse < CC.LDS_HEADS < 2 * sparse
    small = np.zeros(shape, np.uint8)
    small[10:20, 10:40] = 255
    for route in ("0", "1", None):
        if route is None:
            monkeypatch.delenv("VP_CT_MANY", raising=False)
        else:
            monkeypatch.setenv("VP_CT_MANY", route)
        for mode in (0, 1):
            if route is None:
                _check_fit(vp, ctx, oracle, "small", small, mode, 2)        # the context's hint: few heads
                assert _heads(vp, ctx) == CC.head_count(small) < 100
            _check_fit(vp, ctx, oracle, name, m, mode, 2)
            repeated = route is None and H > CC.LDS_HEADS
            assert _heads(vp, ctx) == (sparse if route == "1" or repeated else H), (route, mode)


@pytest.mark.parametrize("form,many", FORMS, ids=[f[0] for f in FORMS])
@pytest.mark.parametrize("N", [127, 128, 255, 256, 257])
def test_hierarchy_around_the_first_capacity(vp, oracle, ctx, monkeypatch, N, form, many):
    """N borders in RETR_CCOMP and RETR_TREE: the wrapper starts with arrays of 256 contours (255, 256, 257: below, at, above; 127 and
    255: max_contours + 1 a power of two, where the sort key of k_ctt_keys gains a bit), then vp_find_contours_tree_u8 with
    max_contours = N - 1, N, N + 1."""
    from vision.utils import feature
    monkeypatch.setenv("VP_CT_MANY", many)
    m = CC.nests_contours(N)
    for mode in (R.RETR_CCOMP, R.RETR_TREE):
        ec, eh, ey = _tree_ref(oracle, ("nc", N), m, mode, 2)
        P = sum(len(c) for c in ec)
        assert len(ec) == N
        feature._capacity.pop(m.shape, None)
        gc, gh, gy = feature.find_contours(m, mode, 2, with_holes=True, with_hierarchy=True)
        assert _same(gc, ec) and np.array_equal(gh, eh) and gy.shape == (1, N, 4) and np.array_equal(gy[0], ey), mode
        for max_c in (N - 1, N, N + 1):
            k, p, pts, counts, holes, hier = _call(vp, ctx, m, mode, 2, max_c, P + 2, "u8", tree=True)
            assert (k, p) == (N, P), (mode, max_c, k, p)
            assert _heads(vp, ctx) == CC.head_count(m, sparse=many == "1")
            if max_c < N:
                assert (counts == FILL).all() and (hier == FILL).all() and (holes == HOLE_FILL).all() and (pts == FILL).all(), (mode, max_c)
                continue
            assert _same(_lists(k, pts, counts), ec) and np.array_equal(holes[:k], eh) and np.array_equal(hier[:k], ey), (mode, max_c)
            assert (counts[max_c:] == FILL).all() and (hier[max_c:] == FILL).all() and (holes[max_c:] == HOLE_FILL).all()
            assert (pts[P + 2:] == FILL).all()


CAPACITY_CASES = [("snake", 1024, 1), ("nests", 1025, 1), ("nests", 1025, 0)]


@pytest.mark.parametrize("form,many", FORMS, ids=[f[0] for f in FORMS])
@pytest.mark.parametrize("entry", ["u8", "dev"])
@pytest.mark.parametrize("fam,H,mode", CAPACITY_CASES, ids=[f"{f}-{h}-mode{md}" for f, h, md in CAPACITY_CASES])
def test_exact_caller_capacities(vp, oracle, ctx, monkeypatch, fam, H, mode, entry, form, many):
    """max_contours in {N - 1, N, N + 1} x max_points in {P - 1, P, P + 1}.  include/vp.h: "*n_contours / *n_points are always the true
    totals; when either exceeds its capacity nothing is copied out" - so the totals are N and P in all nine, the arrays are the oracle's
    when both fit and untouched when one does not, and the sixteen elements behind each capacity are never written."""
    monkeypatch.setenv("VP_CT_MANY", many)
    shape = CC.shape_for(H - H % 1024)
    m = CC.build(fam, H, shape)
    ec, eh, P = _ref(oracle, f"{fam}-{H}", m, mode, 1)
    N = len(ec)
    assert N >= 4 and P > N
    for max_c in (N - 1, N, N + 1):
        for max_p in (P - 1, P, P + 1):
            k, p, pts, counts, holes, _ = _call(vp, ctx, m, mode, 1, max_c, max_p, entry)
            where = (max_c - N, max_p - P)
            assert (k, p) == (N, P), (where, k, p, N, P)
            if max_c < N or max_p < P:
                assert (counts == FILL).all() and (holes == HOLE_FILL).all() and (pts == FILL).all(), where
                continue
            assert _same(_lists(k, pts, counts), ec) and np.array_equal(holes[:k], eh), where
            assert (counts[max_c:] == FILL).all() and (holes[max_c:] == HOLE_FILL).all() and (pts[max_p:] == FILL).all(), where


@pytest.mark.parametrize("mode", [0, 1])
def test_batch_with_frames_on_both_sides(vp, oracle, monkeypatch, mode):
    """1024, 1025, 8192 and 8193 heads side by side in one vp_chain_run_contours call, the masks handed over as they are (grey frames,
    threshold at 128, contours of the threshold mask): a batch never defers, so with one block per frame the fourth works in global
    memory beside three LDS bodies of two instantiations.  Every frame as its own oracle result."""
    from vision.utils import chain, feature
    monkeypatch.setenv("VP_CT_MANY", "0")
    shape = CC.SHAPE_ODD
    masks = [CC.snake(1024, shape), CC.nests(1025, shape), CC.nests(8192, shape), CC.snake(8193, shape)]
    refs = [_ref(oracle, ("batch", i), m, mode, 2) for i, m in enumerate(masks)]
    small = np.zeros(shape, np.uint8)
    small[3, 3] = 255
    assert len(feature.find_contours(small, 1, 2)) == 1               # (the default context's single-image count: one head)
    frames = np.repeat(np.stack(masks)[..., None], 3, axis=3)
    out = chain.run_chain(frames, vp.BGR2GRAY, (128, 0, 0), (255, 255, 255), [], ccl=0, want=("threshed",),
                          contours=dict(source="threshed", mode=mode, method=2, max_contours=max(len(r[0]) for r in refs) + 1,
                                        max_points=max(r[2] for r in refs) + 1))
    for f, (m, (ec, eh, P)) in enumerate(zip(masks, refs)):
        assert np.array_equal(out["threshed"][f], m), f
        got, gh = out["contours"][f]
        assert _same(got, ec) and np.array_equal(gh, eh), (f, len(got), len(ec))
    # the largest head count of the batch, left in pinned memory by its prefix kernel (the call above synchronised)
    assert int(vp.lib().vp_contours_last_heads(vp.default_context().handle)) == CC.LDS_HEADS + 1
