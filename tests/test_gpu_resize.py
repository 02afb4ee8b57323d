"""cv2.resize (INTER_LINEAR, 8-bit) and the letterbox in front of the detector, bit-exact against the statement of OpenCV's resize.cpp
(resize_restate.py) through every entry: cv2_facade.resize with dsize and with fx / fy, utils.transform.resize, vision.yolo.letterbox
on numpy input and on a torch.cuda tensor."""
import numpy as np
import pytest
import torch

import frames as F
import resize_restate as RR
from test_gpu_yolo import _letterbox_ref

pytestmark = pytest.mark.gpu

# (sw, sh) -> (dw, dh) at the edges: 1-pixel sources and destinations, one unchanged axis, exact halvings and doublings, extreme ratios
EDGE_PAIRS = [((1, 1), (7, 5)), ((1, 17), (9, 1)), ((13, 1), (1, 40)), ((300, 200), (1, 1)), ((37, 5), (1, 9)),
              ((123, 45), (123, 77)), ((64, 90), (200, 90)), ((250, 31), (250, 3)), ((200, 100), (100, 50)), ((2, 2), (1, 1)),
              ((298, 2), (149, 1)), ((50, 30), (100, 60)), ((1, 1), (2, 2)), ((1, 1), (300, 300)), ((300, 300), (1, 1)),
              ((1, 300), (300, 1)), ((300, 1), (1, 300)), ((300, 7), (1, 300)), ((3, 3), (300, 2)), ((2, 3), (7, 5))]

# frame sizes the pipeline meets: camera frames to the preprocessor's and the detector's sizes, and back up
REAL_PAIRS = [((1920, 1080), (1366, 768)), ((1920, 1080), (1280, 720)), ((1920, 1080), (960, 540)), ((1920, 1080), (640, 360)),
              ((1920, 1080), (512, 512)), ((1920, 1080), (2048, 2048)), ((1280, 720), (640, 400)), ((3840, 2160), (1920, 1080)),
              ((3840, 2160), (1366, 768)), ((640, 360), (1920, 1080))]

LETTERBOX = [((1080, 1920), (640, 640)), ((360, 640), (640, 640)), ((480, 480), (640, 640)), ((97, 333), (320, 256)),
             ((640, 640), (640, 640)), ((700, 300), (64, 96)), ((720, 1280), (640, 640)), ((1080, 1920), (384, 640)),
             ((2160, 3840), (384, 640)), ((1, 1), (32, 32)), ((300, 1), (64, 64)), ((5, 300), (640, 640))]


def _random_pairs(n=300, seed=2026):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        # half the sides uniform in 1..300, half log-uniform so that small sizes and strong ratios are common
        side = (lambda: int(rng.integers(1, 301))) if i % 2 else (lambda: int(np.exp(rng.uniform(0, np.log(300.5)))))
        out.append(((side(), side()), (side(), side())))
    return out


def _image(rng, w, h, cn):
    img = rng.integers(0, 256, (h, w, cn), dtype=np.uint8)
    return img[:, :, 0].copy() if cn == 1 else img


def _check_all(cases, run):
    """run(case) -> (got, exp); every mismatching case is reported, not only the first."""
    bad = []
    for case in cases:
        got, exp = run(case)
        if got.shape != exp.shape or not np.array_equal(got, exp):
            n = int((got != exp).sum()) if got.shape == exp.shape else -1
            bad.append((case, n))
    assert not bad, f"{len(bad)} of {len(cases)} cases differ from the statement (case, differing values): {bad[:40]}"


def test_facade_dsize_sweep(vp):
    """cv2.resize(src, (dw, dh)): 300 seeded random size pairs plus the edge pairs, cn 1, 3 and 4."""
    from vision import cv2_facade as cv2
    rng = np.random.default_rng(1)
    cases = [(s, d, (1, 3, 4)[i % 3]) for i, (s, d) in enumerate(_random_pairs())]
    cases += [(s, d, cn) for s, d in EDGE_PAIRS for cn in (1, 3, 4)]

    def run(case):
        (sw, sh), (dw, dh), cn = case
        img = _image(rng, sw, sh, cn)
        return cv2.resize(img, (dw, dh)), RR.resize(img, (dw, dh))
    _check_all(cases, run)


def test_facade_real_sizes(vp):
    """The frame sizes of the pipeline, through cv2.resize and utils.transform.resize, on noise and on a rendered scene."""
    from vision import cv2_facade as cv2
    from vision.utils import transform
    rng = np.random.default_rng(2)
    cases = [(s, d, kind) for s, d in REAL_PAIRS for kind in ("noise", "scene")]

    def run(case):
        (sw, sh), (dw, dh), kind = case
        img = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8) if kind == "noise" else F.s1_buoy(3, sw, sh)
        exp = RR.resize(img, (dw, dh))
        got = transform.resize(img, dw, dh) if kind == "scene" else cv2.resize(img, (dw, dh))
        return got, exp
    _check_all(cases, run)


def test_transform_resize_sweep(vp):
    """utils.transform.resize(mat, width, height) on every tenth random pair and the edge pairs, cn 1 and 3."""
    from vision.utils import transform
    rng = np.random.default_rng(3)
    cases = [(s, d, (1, 3)[i % 2]) for i, (s, d) in enumerate(_random_pairs()[::10] + EDGE_PAIRS)]

    def run(case):
        (sw, sh), (dw, dh), cn = case
        img = _image(rng, sw, sh, cn)
        return transform.resize(img, dw, dh), RR.resize(img, (dw, dh))
    _check_all(cases, run)


def _fx_fy_cases():
    rng = np.random.default_rng(4)
    nice = [0.5, 0.25, 1 / 3, 2.0, 1.5, 0.7, 0.1, 3.0, 1.0, 1.01, 0.999, 0.49999999999999994]
    out = []
    for i in range(120):
        sw, sh = int(rng.integers(1, 301)), int(rng.integers(1, 301))
        if i % 3 == 0:
            fx, fy = float(rng.choice(nice)), float(rng.choice(nice))
        else:
            fx, fy = float(np.exp(rng.uniform(np.log(0.05), np.log(4)))), float(np.exp(rng.uniform(np.log(0.05), np.log(4))))
        out.append(((sw, sh), (fx, fy), (1, 3, 4)[i % 3]))
    # issue-style cases: 101 px at fx 0.5 is scale 2 (area-fast) with a partial cell; 100 px at 0.5 is a whole-cell halving
    out += [((100, 60), (0.5, 0.5), 3), ((640, 360), (1 / 3, 1 / 3), 3), ((1, 1), (7.0, 3.0), 1), ((90, 160), (0.7, 1.3), 4)]
    return out


def test_facade_fx_fy(vp):
    """cv2.resize(src, None, fx=fx, fy=fy): dsize = saturate_cast<int>(size * f) and the scale is 1 / f, not size / dsize.  The
    area-fast case with a partial edge cell is not restated and raises cv2.error; an empty destination raises too."""
    from vision import cv2_facade as cv2
    rng = np.random.default_rng(5)
    cases, refused = [], []
    for (sw, sh), (fx, fy), cn in _fx_fy_cases():
        dw, dh = RR.saturate_int(sw * fx), RR.saturate_int(sh * fy)
        partial = (dw, dh) != (sw, sh) and RR.area_fast_2(1 / fx, 1 / fy) and (sw != 2 * dw or sh != 2 * dh)
        (refused if dw <= 0 or dh <= 0 or partial else cases).append(((sw, sh), (fx, fy), cn, (dw, dh)))
    assert len(cases) >= 100 and any(RR.area_fast_2(1 / fx, 1 / fy) for _, (fx, fy), _, _ in cases)

    def run(case):
        (sw, sh), (fx, fy), cn, (dw, dh) = case
        img = _image(rng, sw, sh, cn)
        got = cv2.resize(img, None, fx=fx, fy=fy)
        assert got.shape[:2] == (dh, dw)
        return got, RR.resize(img, None, fx, fy)
    _check_all(cases, run)
    for (sw, sh), (fx, fy), cn, _ in refused:
        with pytest.raises(cv2.error):
            cv2.resize(_image(rng, sw, sh, cn), (0, 0), fx=fx, fy=fy)


def test_area_fast_partial_cell_raises(vp):
    """Scale exactly 2 on both axes with an odd source side: OpenCV's area path would average a partial cell, which is not restated."""
    from vision import cv2_facade as cv2
    img = F.s1_buoy(0, 101, 101)
    for shape in ((101, 101), (100, 101), (101, 100)):
        with pytest.raises(cv2.error):
            cv2.resize(img[:shape[0], :shape[1]].copy(), None, fx=0.5, fy=0.5)
    even = img[:100, :100].copy()
    assert np.array_equal(cv2.resize(even, None, fx=0.5, fy=0.5), RR.area_fast_2x2(even, 50, 50))


@pytest.mark.parametrize("on_device", [False, True])
def test_letterbox_entries(vp, on_device):
    """vision.yolo.letterbox on numpy input and on a torch.cuda tensor against the letterbox of the statement's resize."""
    from vision.yolo import letterbox
    rng = np.random.default_rng(6)
    cases = [(shape, new, "scene") for shape, new in LETTERBOX]
    for _ in range(40):
        cases.append(((int(rng.integers(1, 301)), int(rng.integers(1, 301))), (int(rng.integers(1, 21)) * 32, int(rng.integers(1, 21)) * 32), "noise"))

    def run(case):
        (h, w), new, kind = case
        img = F.s1_buoy(1, w, h) if kind == "scene" and min(h, w) >= 16 else rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        exp, (r, left, top), _ = _letterbox_ref(img, new[0], new[1])
        if on_device:
            got, geom = letterbox(torch.from_numpy(img).cuda(), new)
            got = got.cpu().numpy()
        else:
            got, geom = letterbox(img, new)
        assert abs(geom[0] - r) < 1e-6 and geom[1] == left and geom[2] == top
        return got, exp
    _check_all(cases, run)
