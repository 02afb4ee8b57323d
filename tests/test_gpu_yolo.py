"""Detector pre / post-processing kernels (BASELINE config 5) against plain PyTorch / numpy fp32 restatements of the published
algorithms (LetterBox + preprocess, greedy NMS, probabilistic-IoU rotated NMS).  The third-party package the reference calls
(modules/yolo.py:112) is absent, so parity with it is unpinned; these tests pin the kernels to the restatements."""
import functools

import numpy as np
import pytest
import torch

import frames as F
import resize_restate as RR

pytestmark = pytest.mark.gpu


def _resize_linear_u8(src, nw, nh):
    """cv2.resize(src, (nw, nh), interpolation=INTER_LINEAR) for uint8: the statement of OpenCV's resize.cpp (resize_restate.py)."""
    return RR.resize(src, (nw, nh))


def _letterbox_ref(img, H, W, pad=114):
    h, w = img.shape[:2]
    r = min(H / h, W / w)
    nw, nh = min(max(1, int(round(w * r))), W), min(max(1, int(round(h * r))), H)
    left, top = int(round((W - nw) / 2 - 0.1)), int(round((H - nh) / 2 - 0.1))
    res = img if (nw, nh) == (w, h) else _resize_linear_u8(img, nw, nh)
    canvas = np.full((H, W, 3), pad, np.uint8)
    canvas[top:top + nh, left:left + nw] = res
    chw = np.ascontiguousarray(canvas[:, :, ::-1].transpose(2, 0, 1)).astype(np.float32) / np.float32(255)
    return chw, (r, left, top), (nw, nh)


# The ids are those these shapes had before 480x480 and 97x333 moved to test_letterbox_double_scale_rows below.
@pytest.mark.parametrize("shape,new", [((1080, 1920), (640, 640)), ((360, 640), (640, 640)), ((640, 640), (640, 640)), ((700, 300), (64, 96)),
                                       ((720, 1280), (640, 640))],
                         ids=["shape0-new0", "shape1-new1", "shape4-new4", "shape5-new5", "shape6-new6"])
def test_letterbox(vp, shape, new):
    _check_letterbox(shape, new)


# The two shapes whose expected values changed when the kernels took resize.cpp's double scale and unclamped row weights:
# 480x480 -> 640x640 is an upscale (the first and last rows keep their weight pair on one clipped row), and 97x333 (h x w) fits into
# 75x256, a row scale 97 / 75 that float32 does not hold exactly.
@pytest.mark.parametrize("shape,new", [((480, 480), (640, 640)), ((97, 333), (320, 256))], ids=["480x480-640x640", "97x333-320x256"])
def test_letterbox_double_scale_rows(vp, shape, new):
    _check_letterbox(shape, new)


# Content or source of one row / column (rs_row / rs_col with ssize == 1, P.nh == 1, P.nw == 1), a 1 x 1 source, and an exact doubling,
# which must take the generic path (the 2 x 2 average belongs to the exact halving alone).
@pytest.mark.parametrize("shape,new", [((1, 500), (64, 64)), ((500, 1), (64, 64)), ((1, 1), (32, 48)), ((2, 2), (4, 4)), ((3, 1000), (64, 64))],
                         ids=["1x500-64x64", "500x1-64x64", "1x1-32x48", "2x2-4x4", "3x1000-64x64"])
def test_letterbox_edges(vp, shape, new):
    _check_letterbox(shape, new)


def _check_letterbox(shape, new):
    from vision.yolo import letterbox
    img = F.s1_buoy(1, shape[1], shape[0])
    got, geom = letterbox(img, new)
    exp, (r, left, top), (nw, nh) = _letterbox_ref(img, new[0], new[1])
    assert got.shape == (3, new[0], new[1]) and got.dtype == np.float32
    assert abs(geom[0] - r) < 1e-6 and geom[1] == left and geom[2] == top
    assert np.array_equal(got, exp)                              # same fixed-point arithmetic as the restatement
    # independent witness: float bilinear interpolation with half-pixel centres (torch), within the 8-bit rounding of the resize
    t = torch.from_numpy(np.ascontiguousarray(img[:, :, ::-1].transpose(2, 0, 1)).astype(np.float32))[None]
    ref = torch.nn.functional.interpolate(t, size=(nh, nw), mode="bilinear", align_corners=False)[0].numpy() / 255.0
    inner = got[:, top:top + nh, left:left + nw]
    assert np.abs(inner - ref).max() <= 1.01 / 255
    pad = np.ones((new[0], new[1]), bool)
    pad[top:top + nh, left:left + nw] = False
    assert (got[:, pad] == np.float32(114) / np.float32(255)).all()
    # device entry: torch tensor in, torch tensor out, same values
    g2, geom2 = letterbox(torch.from_numpy(img).cuda(), new)
    assert g2.is_cuda and np.array_equal(g2.cpu().numpy(), got) and geom2 == geom


def _iou(a, b):
    ix = np.maximum(np.float32(0), np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0]))
    iy = np.maximum(np.float32(0), np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1]))
    inter = ix * iy
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) - inter)


def _score_order(scores):
    """Indices in the kernels' score order: numbers descending (+inf first, -inf last, -0.0 == 0.0 a tie), every number before every
    NaN, ties and NaNs among themselves by lower index.  np.lexsort already is that order: it sorts -scores ascending with NaN last
    (numpy's sort order puts NaN after every number, +inf included) and, being stable on its last key, leaves equal keys and the
    NaNs to the index."""
    return np.lexsort((np.arange(len(scores)), -scores))


def _nms_ref(boxes, scores, thr, max_det):
    order = _score_order(scores)                                   # score descending, ties by index, NaN last
    alive = np.ones(len(order), bool)
    keep = []
    for pos, i in enumerate(order):
        if not alive[pos]:
            continue
        keep.append(i)
        if len(keep) == max_det:
            break
        rest = order[pos + 1:]
        alive[pos + 1:] &= ~(_iou(boxes[i], boxes[rest]) > np.float32(thr))
    return np.array(keep, np.int64)


def _boxes(rng, n, size=640):
    c = rng.uniform(0, size, (n, 2)).astype(np.float32)
    wh = rng.uniform(4, 200, (n, 2)).astype(np.float32)
    return np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 300, 2000, 8400])
def test_nms_greedy(vp, n):
    from vision.yolo import nms
    rng = np.random.default_rng(n)
    boxes = _boxes(rng, n)
    scores = rng.random(n).astype(np.float32)
    if n > 10:
        scores[5] = scores[3]                                      # a tie
        boxes[7] = boxes[2]                                        # exact duplicates
    for thr in (0.3, 0.45, 0.7):
        got = nms(boxes, scores, thr, max_det=300)
        exp = _nms_ref(boxes, scores, thr, 300)
        assert np.array_equal(got, exp), (n, thr)
    if n:
        assert np.array_equal(nms(boxes, scores, 0.45, max_det=3), _nms_ref(boxes, scores, 0.45, 3))
        g = nms(torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), 0.45, max_det=300)
        assert g.is_cuda and np.array_equal(g.cpu().numpy(), _nms_ref(boxes, scores, 0.45, 300))


# How far test_nms_greedy's two large cases reach with max_det = 300 (the reference alone, at those seeds): _nms_ref returns 300 boxes
# in all six, and the 300th survivor, after which k_nms_greedy leaves its loop, sits at the sorted position
#     n = 2000:  631 (thr 0.3), 386 (thr 0.45), 309 (thr 0.7)          n = 8400:  617, 387, 303
# so no position from 632 on was ever visited.  Without the cut there are 667 / 1081 / 1845 survivors (n = 2000) and 1596 / 2919 / 6583
# (n = 8400), the last of them at the sorted positions 1998 / 1998 / 1999 and 8396 / 8396 / 8398.
@pytest.mark.parametrize("n", [2000, 8400])
def test_nms_greedy_uncut(vp, n):
    """test_nms_greedy's random boxes with max_det = n: the greedy pass walks every sorted position."""
    from vision.yolo import nms
    rng = np.random.default_rng(n)
    boxes = _boxes(rng, n)
    scores = rng.random(n).astype(np.float32)
    scores[5] = scores[3]
    boxes[7] = boxes[2]
    for thr in (0.3, 0.45, 0.7):
        exp = _nms_ref(boxes, scores, thr, n)
        assert np.array_equal(nms(boxes, scores, thr, max_det=n), exp), (n, thr)
    g = nms(torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), 0.7, max_det=n)
    assert g.is_cuda and np.array_equal(g.cpu().numpy(), exp)


def _probiou(b1, b2, eps=1e-7):
    def cov(b):
        a, bb, c = b[:, 2:3] ** 2 / 12, b[:, 3:4] ** 2 / 12, b[:, 4:5]
        cos, sin = c.cos(), c.sin()
        return a * cos ** 2 + bb * sin ** 2, a * sin ** 2 + bb * cos ** 2, (a - bb) * cos * sin
    x1, y1 = b1[:, 0:1], b1[:, 1:2]
    x2, y2 = b2[:, 0][None], b2[:, 1][None]
    a1, bb1, c1 = cov(b1)
    a2, bb2, c2 = (t[:, 0][None] for t in cov(b2))
    den = (a1 + a2) * (bb1 + bb2) - (c1 + c2) ** 2
    t1 = (((a1 + a2) * (y1 - y2) ** 2 + (bb1 + bb2) * (x1 - x2) ** 2) / (den + eps)) * 0.25
    t2 = (((c1 + c2) * (x2 - x1) * (y1 - y2)) / (den + eps)) * 0.5
    t3 = (den / (4 * ((a1 * bb1 - c1 ** 2).clamp(min=0) * (a2 * bb2 - c2 ** 2).clamp(min=0)).sqrt() + eps) + eps).log() * 0.5
    bd = (t1 + t2 + t3).clamp(eps, 100.0)
    return 1 - (1.0 - (-bd).exp() + eps).sqrt()


@pytest.mark.parametrize("n", [1, 50, 700, 3000])
def test_nms_rotated(vp, n):
    """Probabilistic IoU + the rule 'drop a box when some higher-scored box overlaps it by >= thr' (torch fp32 restatement).  The
    kernel's float32 ops are the same formula in a different evaluation order, so boxes whose overlap with the decisive
    neighbour lies within 1e-4 of the threshold are allowed to differ."""
    from vision.yolo import nms_rotated
    rng = np.random.default_rng(100 + n)
    xywh = np.concatenate([rng.uniform(0, 640, (n, 2)), rng.uniform(8, 160, (n, 2))], 1)
    boxes = np.concatenate([xywh, rng.uniform(-np.pi / 2, np.pi / 2, (n, 1))], 1).astype(np.float32)
    scores = rng.random(n).astype(np.float32)
    thr = 0.45
    got = set(nms_rotated(boxes, scores, thr, max_det=n).tolist())
    order = np.lexsort((np.arange(n), -scores))
    tb = torch.from_numpy(boxes[order])
    ious = _probiou(tb, tb).triu_(diagonal=1)
    mx = ious.max(dim=0)[0].numpy()
    exp = set(order[mx < thr].tolist())
    unsure = set(order[np.abs(mx - thr) < 1e-4].tolist())
    # The restatement alone gives 0, 0, 0, 2 such boxes for n = 1, 50, 700, 3000 at these seeds.  The cap is no tolerance: it keeps the
    # allowance from growing until it hides a kernel that disagrees on many boxes.
    assert len(unsure) <= 4
    assert (got ^ exp) <= unsure, (len(got ^ exp), len(unsure))
    kept = nms_rotated(boxes, scores, thr, max_det=n)
    assert list(scores[kept]) == sorted(scores[kept], reverse=True)       # best score first
    if n > 1:
        g = nms_rotated(torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), thr, max_det=n)
        assert set(g.cpu().numpy().tolist()) == got


# ---- constructions whose answer is known without any suppression code --------------------------------------------------------------
# Clusters: box i belongs to cluster i // 16; the boxes of a cluster nearly coincide, clusters lie a pitch apart that is well over the
# box side.  Whatever the rule (greedy or "worse than some higher-scored box"), what survives is the best-scored box of every cluster,
# best first.  The first n boxes of a construction are a construction again (the last cluster may be short).
NMS_CAP = 16384                      # vp_nms_*: n <= 16384
_PER = 16                            # boxes per cluster
_SLOTS = (4096, 8192, 12288)         # first sorted position of k_nms_greedy's rem[1], rem[2], rem[3]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                                  # (a copy: the shared constructions are read-only)


def _cluster_scores(rng, n, spread):
    """n distinct float32 scores k / n, k = 1..n, as a random permutation.  spread = False: a uniform one.  The best box of a cluster
    of 16 then sits early in the order (beyond the first half for about one cluster in 2^16), so late sorted positions are all
    suppressed ones.  spread = True: cluster c draws its ranks from [u_c n, n) with u_c uniform, so the winners - the candidates the
    greedy pass keeps and whose mask row it reads - lie at all sorted positions, and their clusters reach from there to the end."""
    k = np.arange(n, 0, -1).astype(np.float32) / np.float32(n)                   # descending
    if not spread:
        return k[rng.permutation(n)]
    u = np.repeat(rng.random((n + _PER - 1) // _PER), _PER)[:n]
    s = np.empty(n, np.float32)
    s[np.argsort(u + (1 - u) * rng.random(n))] = k
    return s


def _cluster_winners(scores):
    order = _score_order(scores)
    _, first = np.unique(order // _PER, return_index=True)        # first sorted position of every cluster
    return order[np.sort(first)]


def _grid_centres(n, cols, pitch):
    c = np.arange((n + _PER - 1) // _PER)
    return np.repeat((np.stack([c % cols, c // cols], 1) * pitch + pitch // 2).astype(np.float32), _PER, 0)[:n]


@functools.lru_cache(maxsize=None)
def _clustered_xyxy(spread):
    """16384 boxes of side 40 +- 0.5 per edge, 1024 centres at pitch 64, and scores; checked here, on the CPU, with _iou: every pair
    within a cluster overlaps by more than 0.75 (worst case 39^2 / (2 * 41^2 - 39^2) = 0.826), every pair across clusters by exactly 0
    (the gap is at least 64 - 41, and 0 * iy / union = 0)."""
    rng = np.random.default_rng(16384 + int(spread))
    centre = _grid_centres(NMS_CAP, 32, 64)
    boxes = (np.concatenate([centre - 20, centre + 20], 1) + rng.uniform(-0.5, 0.5, (NMS_CAP, 4))).astype(np.float32)
    scores = _cluster_scores(rng, NMS_CAP, spread)
    assert len(np.unique(scores)) == NMS_CAP
    members = boxes.reshape(-1, _PER, 4).transpose(1, 2, 0)                      # (16, 4, clusters)
    assert min(float(_iou(members[k], members).min()) for k in range(_PER)) > 0.7 + 0.05
    # across clusters: the bounds of a cluster (smallest x1, y1, largest x2, y2 of its boxes) against those of every other.  Where two
    # bounds have ix == 0 (or iy == 0), min(a[2], b[2]) - max(a[0], b[0]) is no larger for any box a of the one and b of the other
    # (min, max and the rounded difference are monotone), so all 2^28 pairs have an intersection, and an IoU, of exactly 0.
    per = boxes.reshape(-1, _PER, 4)
    bounds = np.concatenate([per[:, :, :2].min(1), per[:, :, 2:].max(1)], 1)
    cross = _iou(bounds.T[:, :, None], bounds)                                   # (1024, 1024)
    assert (np.diag(cross) == 1).all() and np.count_nonzero(cross) == len(bounds)
    return _frozen(boxes, scores)


@pytest.mark.parametrize("spread", [False, True], ids=["uniform", "spread"])
@pytest.mark.parametrize("n", [4095, 4096, 4097, 8192, 12288, 12289, 16383, 16384])
def test_nms_greedy_clusters_to_capacity(vp, n, spread):
    """Up to the kernel's capacity with max_det = n, so k_nms_greedy walks all sorted positions: every slot of its register bitmap
    (rem[i >> 12]), every word of the mask rows, and k_nms_mask's late rows.  Expected without any suppression code: the best box
    of every cluster, best first."""
    from vision.yolo import nms
    boxes, scores = (a[:n] for a in _clustered_xyxy(spread))
    exp = _cluster_winners(scores)
    assert len(exp) == (n + _PER - 1) // _PER
    pos = np.flatnonzero(np.isin(_score_order(scores), exp))                     # sorted positions of the survivors
    for b in _SLOTS:
        if spread and n >= b + 64:                                               # a kept candidate on either side of the slot boundary
            assert (pos < b).any() and (pos >= b).sum() >= 4, (b, (pos >= b).sum())
    assert np.array_equal(_nms_ref(boxes, scores, 0.7, n), exp)
    assert np.array_equal(nms(boxes, scores, 0.7, max_det=n), exp)
    g = nms(_dev(boxes), _dev(scores), 0.7, max_det=n)
    assert g.is_cuda and np.array_equal(g.cpu().numpy(), exp)


def test_nms_over_capacity_is_refused(vp):
    n = NMS_CAP + 1
    rng = np.random.default_rng(n)
    from vision.yolo import nms, nms_rotated
    for fn, bs in ((nms, 4), (nms_rotated, 5)):
        boxes = np.concatenate([_boxes(rng, n), np.zeros((n, bs - 4), np.float32)], 1)
        scores = rng.random(n).astype(np.float32)
        with pytest.raises(vp.VpError, match=r"\(%d\).*16384" % vp.ERR_UNSUPPORTED):
            fn(boxes, scores, 0.7, max_det=300)
        with pytest.raises(vp.VpError, match=r"\(%d\).*16384" % vp.ERR_UNSUPPORTED):
            fn(torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), 0.7, max_det=300)
    assert np.array_equal(nms(boxes[:3, :4], scores[:3], 0.7), _nms_ref(boxes[:3, :4], scores[:3], 0.7, 300))   # the context still works


def _rot_worst(boxes, scores, chunk=512):
    """(order, worst): worst[k] = the largest probabilistic IoU of the box at sorted position k with a box before it (0 if none) -
    test_nms_rotated's `_probiou(tb, tb).triu_(1).max(0)`, columns `chunk` at a time.  A box survives when worst < thr."""
    order = _score_order(scores)
    tb = torch.from_numpy(boxes[order])
    n = len(order)
    worst = np.zeros(n, np.float32)
    for j0 in range(0, n, chunk):
        j1 = min(n, j0 + chunk)
        iou = _probiou(tb[:j1], tb[j0:j1])                                       # rows: sorted positions 0..j1, the higher-scored side
        iou[j0:] = iou[j0:].triu(diagonal=1)
        worst[j0:j1] = iou.max(dim=0)[0].clamp(min=0).numpy()
    return order, worst


def _rot_ref(boxes, scores, thr, max_det):
    """-> (kept, best first; the boxes within 1e-4 of the threshold, which may fall either way)"""
    order, worst = _rot_worst(boxes, scores)
    return order[worst < thr][:max_det], order[np.abs(worst - thr) < 1e-4]


def _clustered_xywhr(rng, n, cols, spread=False):
    """n rotated boxes (x, y, w, h, angle) in clusters at pitch 128: per cluster one shape (60 x 30 or 30 x 60) and one angle with
    0.1 <= |angle| <= 1.4 (so no regularised angle lies next to the wrap at 0 / pi), per box +- 0.5 on x, y, w, h and +- 0.01 rad."""
    ncl = (n + _PER - 1) // _PER
    wh = np.where(rng.random(ncl)[:, None] < 0.5, [[60.0, 30.0]], [[30.0, 60.0]])
    ang = rng.uniform(0.1, 1.4, ncl) * rng.choice([-1.0, 1.0], ncl)
    per = np.repeat(np.concatenate([wh, ang[:, None]], 1), _PER, 0)[:n]
    boxes = np.concatenate([_grid_centres(n, cols, 128), per], 1)
    boxes += np.concatenate([rng.uniform(-0.5, 0.5, (n, 4)), rng.uniform(-0.01, 0.01, (n, 1))], 1)
    return boxes.astype(np.float32), _cluster_scores(rng, n, spread)


def _check_rot_clusters(boxes, thr, cl=None, chunk=512):
    """On the CPU with _probiou, over all ordered pairs: within a cluster >= thr + 0.05, across clusters <= thr - 0.05 (so no pair is
    anywhere near the threshold, whichever of the two scores higher).  cl: the cluster of every box (default: index // 16)."""
    tb = torch.from_numpy(boxes)
    cl = torch.arange(len(boxes)) // _PER if cl is None else torch.from_numpy(cl)
    for j0 in range(0, len(boxes), chunk):
        iou = _probiou(tb, tb[j0:j0 + chunk])
        same = cl[:, None] == cl[None, j0:j0 + chunk]
        assert float(iou[same].min()) >= thr + 0.05 and float(iou[~same].max()) <= thr - 0.05


@functools.lru_cache(maxsize=None)
def _rot_case(n):
    rng = np.random.default_rng(500 + n)
    boxes, scores = _clustered_xywhr(rng, n, 32, spread=True)
    _check_rot_clusters(boxes, 0.5)
    return _frozen(boxes, scores)


@pytest.mark.parametrize("n", [3000, 8192])
def test_nms_rotated_clusters_order_and_cut(vp, n):
    """The kept list itself, not its set: in full (max_det = n), and cut in the middle of one of k_nms_compact's groups of 64 sorted
    positions with survivors on both sides of the cut inside that group."""
    from vision.yolo import nms_rotated
    thr = 0.5
    boxes, scores = _rot_case(n)
    exp = _cluster_winners(scores)
    ref, unsure = _rot_ref(boxes, scores, thr, n)
    assert len(unsure) == 0 and np.array_equal(ref, exp)
    assert np.array_equal(nms_rotated(boxes, scores, thr, max_det=n), exp)
    alive = np.isin(_score_order(scores), exp)                                   # by sorted position
    k = next(k for k in range(2, n // 64) if alive[64 * k:64 * k + 32].any() and alive[64 * k + 32:64 * k + 64].any())
    cut = int(alive[:64 * k + 32].sum())
    assert 0 < cut < len(exp)
    tb, ts = _dev(boxes), _dev(scores)
    for max_det in (cut, n):
        assert np.array_equal(nms_rotated(boxes, scores, thr, max_det=max_det), exp[:max_det]), max_det
        g = nms_rotated(tb, ts, thr, max_det=max_det)
        assert g.is_cuda and np.array_equal(g.cpu().numpy(), exp[:max_det]), max_det


def test_nms_chains(vp):
    """A = [0, 10], B = [5, 15], C = [10, 20] along x, all 10 high, scores A > B > C: IoU(A, B) = IoU(B, C) = 1 / 3, A and C share an
    edge only.  Greedy: A drops B, and B, being dropped, drops nothing: [A, C].  The rotated rule asks for any higher-scored box,
    dropped or not: [A]."""
    from vision.yolo import nms, nms_rotated
    t, thr = 300, 0.25
    rng = np.random.default_rng(7)
    origin = np.repeat(np.stack([np.arange(t) % 20, np.arange(t) // 20], 1) * 64.0, 3, 0)
    x0 = np.tile([0.0, 5.0, 10.0], t)
    xyxy = np.stack([origin[:, 0] + x0, origin[:, 1], origin[:, 0] + x0 + 10, origin[:, 1] + 10], 1).astype(np.float32)
    base = np.repeat(rng.permutation(t), 3) * 3 + np.tile([2, 1, 0], t)          # distinct; A > B > C inside every triple
    scores = (base + 1).astype(np.float32) / np.float32(3 * t)
    for a, b, c in ((0, 1, 1.0 / 3), (1, 2, 1.0 / 3), (0, 2, 0.0)):
        iou = np.array([_iou(xyxy[3 * i + a], xyxy[3 * i + b:3 * i + b + 1])[0] for i in range(t)])
        assert (np.abs(iou - c) < 1e-6).all() and ((iou > thr + 0.05) if c else (iou == 0)).all()
    xywhr = np.concatenate([(xyxy[:, :2] + xyxy[:, 2:]) / 2, xyxy[:, 2:] - xyxy[:, :2], np.zeros((3 * t, 1), np.float32)], 1).astype(np.float32)
    p = _probiou(torch.from_numpy(xywhr[:3]), torch.from_numpy(xywhr[:3])).numpy()    # the triples are translates of the first
    assert p[0, 1] > thr + 0.05 and p[1, 2] > thr + 0.05 and p[0, 2] < thr - 0.05
    shuffle = rng.permutation(3 * t)
    xyxy, xywhr, scores, role = xyxy[shuffle], xywhr[shuffle], scores[shuffle], np.tile([0, 1, 2], t)[shuffle]
    order = _score_order(scores)
    exp_greedy, exp_rot = order[role[order] != 1], order[role[order] == 0]
    assert np.array_equal(_nms_ref(xyxy, scores, thr, 3 * t), exp_greedy)
    ref, unsure = _rot_ref(xywhr, scores, thr, 3 * t)
    assert len(unsure) == 0 and np.array_equal(ref, exp_rot)
    assert np.array_equal(nms(xyxy, scores, thr, max_det=3 * t), exp_greedy)
    assert np.array_equal(nms_rotated(xywhr, scores, thr, max_det=3 * t), exp_rot)
    assert np.array_equal(nms(torch.from_numpy(xyxy).cuda(), torch.from_numpy(scores).cuda(), thr, max_det=3 * t).cpu().numpy(), exp_greedy)
    assert np.array_equal(nms_rotated(torch.from_numpy(xywhr).cuda(), torch.from_numpy(scores).cuda(), thr, max_det=3 * t).cpu().numpy(), exp_rot)


def test_nms_threshold_direction_and_duplicates(vp):
    """Greedy drops on IoU > thr, not >=.  [0, 0, 4, 4] and [0, 0, 4, 2]: intersection 8, union 16 + 8 - 8, IoU = 0.5 with every
    intermediate a small integer - exact in float32 however the compiler arranges the arithmetic."""
    from vision.yolo import nms, nms_rotated
    boxes = np.array([[0, 0, 4, 4], [0, 0, 4, 2]], np.float32)
    scores = np.array([0.9, 0.8], np.float32)
    assert _iou(boxes[0], boxes[1:])[0] == np.float32(0.5)
    below = np.nextafter(np.float32(0.5), np.float32(0))
    assert float(below) < 0.5 and np.float32(float(below)) == below
    for dev in (False, True):
        b, s = (torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()) if dev else (boxes, scores)
        out = (lambda r: r.cpu().numpy()) if dev else (lambda r: r)
        assert out(nms(b, s, 0.5)).tolist() == [0, 1]                            # 0.5 > 0.5 is false: both stay
        assert out(nms(b, s, float(below))).tolist() == [0]
        assert out(nms(b.flip(0) if dev else b[::-1], s, float(below))).tolist() == [0]       # (whichever of the two scores higher)
    # exact duplicates with equal scores: the lower index stays, under either rule
    rng = np.random.default_rng(11)
    n = 200
    xyxy = _boxes(rng, n)
    xywhr = np.concatenate([rng.uniform(0, 6400, (n, 2)), rng.uniform(8, 40, (n, 2)), rng.uniform(-1.5, 1.5, (n, 1))], 1).astype(np.float32)
    scores = _cluster_scores(rng, n, False)
    pairs = ((3, 150), (64, 65), (10, 199))
    for lo, hi in pairs:
        xyxy[hi], xywhr[hi], scores[hi] = xyxy[lo], xywhr[lo], scores[lo]
    got = nms(xyxy, scores, 0.45, max_det=n)
    assert np.array_equal(got, _nms_ref(xyxy, scores, 0.45, n))
    ref, unsure = _rot_ref(xywhr, scores, 0.45, n)
    got_r = nms_rotated(xywhr, scores, 0.45, max_det=n)
    assert len(unsure) == 0 and np.array_equal(got_r, ref)
    assert not any(hi in got or hi in got_r for _, hi in pairs)
    assert any(lo in got for lo, _ in pairs) and any(lo in got_r for lo, _ in pairs)


def _special_scores(rng, n):
    """About 3 % NaN at random positions, index 0 and n - 1 among them, a +inf, a -inf and a 0.0 / -0.0 pair."""
    scores = rng.random(n).astype(np.float32)
    idx = rng.permutation(np.arange(1, n - 1))
    nan = np.concatenate([[0, n - 1], idx[:max(2, (3 * n) // 100)]])
    a, b, c, d = idx[-4:]
    scores[nan] = np.nan
    scores[a], scores[b], scores[c], scores[d] = np.inf, -np.inf, 0.0, -0.0
    return scores, (a, b, c, d)


@pytest.mark.parametrize("n", [300, 4200])
def test_nms_nan_and_special_scores(vp, n):
    """k_nms_rank's order is total: a number before a NaN, NaNs by index, -0.0 == 0.0 a tie.  Every slot of order[] is written once,
    which shows as indices that are in range and unique; a NaN-scored box is a candidate like any other, at the end."""
    from vision.yolo import nms, nms_rotated
    rng = np.random.default_rng(900 + n)
    xyxy = _boxes(rng, n, size=2000)
    scores, (pinf, ninf, pz, nz) = _special_scores(rng, n)
    order = _score_order(scores)
    nn = int(np.isnan(scores).sum())
    assert nn >= 0.03 * n and np.isnan(scores[[0, n - 1]]).all()
    assert order[0] == pinf and order[n - nn - 1] == ninf and np.array_equal(order[n - nn:], np.flatnonzero(np.isnan(scores)))
    assert abs(int(np.flatnonzero(order == pz)[0]) - int(np.flatnonzero(order == nz)[0])) == 1      # a tie: neighbours, by index
    assert (np.flatnonzero(order == pz)[0] < np.flatnonzero(order == nz)[0]) == (pz < nz)
    rot, rot_scores = _clustered_xywhr(np.random.default_rng(950 + n), n, 32)
    _check_rot_clusters(rot, 0.5)
    rot_scores = np.where(np.isnan(scores) | np.isinf(scores) | (scores == 0), scores, rot_scores)
    c = n // _PER - 2
    rot_scores[_PER * c:_PER * (c + 1)] = np.nan                                 # a cluster of NaNs only: its lowest index survives
    exp_g = _nms_ref(xyxy, scores, 0.45, n)
    exp_r, unsure = _rot_ref(rot, rot_scores, 0.5, n)
    assert len(unsure) == 0 and np.array_equal(exp_r, _cluster_winners(rot_scores))
    assert np.isnan(scores[exp_g]).any() and np.isnan(rot_scores[exp_r]).any()  # some NaN-scored box is kept under either rule
    for dev in (False, True):
        up = (lambda a: torch.from_numpy(a).cuda()) if dev else (lambda a: a)
        out = (lambda r: r.cpu().numpy()) if dev else (lambda r: r)
        for got, exp in ((out(nms(up(xyxy), up(scores), 0.45, max_det=n)), exp_g),
                         (out(nms_rotated(up(rot), up(rot_scores), 0.5, max_det=n)), exp_r),
                         (out(nms(up(xyxy), up(scores), 0.45, max_det=len(exp_g) - 1)), exp_g[:-1])):
            assert ((got >= 0) & (got < n)).all() and len(np.unique(got)) == len(got), dev
            assert np.array_equal(got, exp), dev


def test_nms_all_scores_nan(vp):
    from vision.yolo import nms, nms_rotated
    n = 300
    rng = np.random.default_rng(77)
    xyxy = _boxes(rng, n, size=2000)
    rot, _ = _clustered_xywhr(rng, n, 32)
    scores = np.full(n, np.nan, np.float32)
    assert np.array_equal(_score_order(scores), np.arange(n))
    exp_g = _nms_ref(xyxy, scores, 0.45, n)
    exp_r, unsure = _rot_ref(rot, scores, 0.5, n)
    assert len(unsure) == 0 and np.array_equal(exp_r, np.arange(0, n, _PER))     # the lowest index of every cluster
    assert (np.diff(exp_g) > 0).all() and exp_g[0] == 0
    for dev in (False, True):
        up = (lambda a: torch.from_numpy(a).cuda()) if dev else (lambda a: a)
        out = (lambda r: r.cpu().numpy()) if dev else (lambda r: r)
        assert np.array_equal(out(nms(up(xyxy), up(scores), 0.45, max_det=n)), exp_g)
        assert np.array_equal(out(nms_rotated(up(rot), up(scores), 0.5, max_det=n)), exp_r)


def test_postprocess_caps_candidates_at_capacity(vp):
    """20000 candidates above the confidence threshold: Detector.postprocess suppresses among the 16384 most confident (the kernel's
    capacity) instead of raising.  1250 clusters of 16, one class each; the 1600 least confident candidates are the last 100 clusters,
    which therefore yield nothing - a cut by position instead of by confidence would keep them."""
    from vision.yolo.engine import MAX_NMS, YOLO
    assert MAX_NMS == NMS_CAP
    n, nc, thr = 20000, 15, 0.7
    m = YOLO(None, conf=0.0, iou=thr, max_det=2000).to("cuda")                   # random-init model, as test_gpu_yolo_module builds it
    assert len(m.names) == nc
    rng = np.random.default_rng(20000)
    boxes, _ = _clustered_xywhr(rng, n, 40)
    cls = (np.arange(n) // _PER) % nc
    conf = np.empty(n, np.float32)
    k = np.arange(1, n + 1).astype(np.float32) / np.float32(n)                   # distinct, all above conf = 0
    conf[:n - 1600] = k[1600:][rng.permutation(n - 1600)]
    conf[n - 1600:] = k[:1600][rng.permutation(1600)]
    pred = np.zeros((4 + nc + 1, n), np.float32)
    pred[:4], pred[-1] = boxes[:, :4].T, boxes[:, 4]
    pred[4 + cls, np.arange(n)] = conf
    geom = (2.0, 3.0, 12.0)                      # (results below 2600: float32 keeps them to 3e-4, the comparison asks for 1e-3)
    res = m.postprocess(torch.from_numpy(pred).cuda(), geom, (720, 1280, 3))
    # restatement: the MAX_NMS best by confidence, other classes 7680 away, the rotated rule, regularise, undo the letterbox
    sel = _score_order(conf)[:NMS_CAP]
    assert sel.max() < n - 1600
    shifted = boxes[sel].copy()
    shifted[:, :2] += (cls[sel].astype(np.float32) * np.float32(7680.0))[:, None]
    # The classes' candidates lie more than 2000 px apart in x (sides are 61 at most): across classes the probabilistic IoU is 0 to
    # the last bit (the distance term runs into its clamp at 100), so the rule is applied class by class - 15 x 1100^2 pairs, not 16384^2
    lo, hi = (np.array([f(shifted[cls[sel] == c, 0]) for c in range(nc)]) for f in (np.min, np.max))
    assert (lo[1:] - hi[:-1] > 2000).all()
    kept = []
    for c in range(nc):
        of_c = np.flatnonzero(cls[sel] == c)
        _check_rot_clusters(shifted[of_c], thr, cl=sel[of_c] // _PER)
        kept_c, unsure = _rot_ref(shifted[of_c], conf[sel][of_c], thr, n)
        assert len(unsure) == 0                                                 # by construction: no pair is within 0.05 of the threshold
        kept.append(sel[of_c[kept_c]])
    kept = np.concatenate(kept)
    kept = kept[_score_order(conf[kept])][:m.max_det]
    assert np.array_equal(np.sort(kept // _PER), np.arange((n - 1600) // _PER))  # one per cluster that has a candidate among the best
    x, y, w, h, t = boxes[kept].astype(np.float64).T
    swap = h > w
    exp = np.stack([(x - geom[1]) / geom[0], (y - geom[2]) / geom[0], np.where(swap, h, w) / geom[0], np.where(swap, w, h) / geom[0],
                    np.where(swap, t + np.pi / 2, t) % np.pi], 1)
    assert len(res) == len(kept) and np.array_equal(res.cls, cls[kept]) and np.array_equal(res.conf, conf[kept])
    assert np.allclose(res.boxes, exp, rtol=0, atol=1e-3)
    v1 = np.stack([exp[:, 2] / 2 * np.cos(exp[:, 4]), exp[:, 2] / 2 * np.sin(exp[:, 4])], 1)
    v2 = np.stack([-exp[:, 3] / 2 * np.sin(exp[:, 4]), exp[:, 3] / 2 * np.cos(exp[:, 4])], 1)
    ctr = exp[:, :2]
    assert np.allclose(res.corners, np.stack([ctr + v1 + v2, ctr + v1 - v2, ctr - v1 - v2, ctr - v1 + v2], 1), rtol=0, atol=1e-2)


def test_detection_records_and_corner_order(vp):
    from vision.yolo import OBBData, order_points, scale_boxes
    d = OBBData("torpedo_board", 0.9, 10, 5, 110, 8, 108, 60, 12, 58)
    tl, tr, bl, br = order_points([(d.x1, d.y1), (d.x2, d.y2), (d.x3, d.y3), (d.x4, d.y4)])
    assert tl == (10, 5) and tr == (110, 8) and br == (108, 60) and bl == (12, 58)
    b = scale_boxes(np.array([[100, 140, 300, 340]], np.float32), (0.5, 0, 140))
    assert np.allclose(b, [[200, 0, 600, 400]])


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_resize_linear_u8_statement(vp, cn):
    """cv2.resize (facade) == the statement of resize.cpp (double scale, unclamped row weights), and within one count of float
    bilinear interpolation."""
    from vision import cv2_facade as cv2
    rng = np.random.default_rng(cn)
    for (h, w), (dh, dw) in [((90, 160), (45, 80)), ((90, 160), (512, 512)), ((33, 65), (7, 200)), ((64, 64), (64, 64)), ((100, 50), (99, 51))]:
        img = rng.integers(0, 256, (h, w, cn), dtype=np.uint8)
        src = img[:, :, 0] if cn == 1 else img
        got = cv2.resize(src, (dw, dh))
        exp = _resize_linear_u8(img, dw, dh)
        assert got.shape == ((dh, dw) if cn == 1 else (dh, dw, cn))
        assert np.array_equal(got.reshape(dh, dw, cn), exp)
        t = torch.from_numpy(img.transpose(2, 0, 1).astype(np.float32))[None]
        ref = torch.nn.functional.interpolate(t, size=(dh, dw), mode="bilinear", align_corners=False)[0].numpy().transpose(1, 2, 0)
        assert np.abs(got.reshape(dh, dw, cn).astype(np.float32) - ref).max() <= 1.01
