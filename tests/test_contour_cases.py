"""CPU: the head count restated in tests/contour_cases.py against values derived by hand, and every mask the GPU tests of the contour
pass use (tests/test_gpu_contour_capacity.py), built here once so that each builder's count is checked without a GPU."""
import os
import re

import numpy as np
import pytest

import contour_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc", "vp_contours.inl")).read()
_PLAN = open(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc", "vp_contours_plan.h")).read()      # the constants host and device share


def _mask(h, w, pixels):
    m = np.zeros((h, w), np.uint8)
    for y, x in pixels:
        m[y, x] = 255
    return m


def test_constants_are_the_kernels():
    """the boundaries of the cases are the ones k_ct_jump compares the head count with"""
    assert int(re.search(r"#define CTJ_LDS_HEADS (\d+)", _PLAN).group(1)) == CC.LDS_HEADS == CC.BOUNDARIES[-1]
    assert "#define CTJ_LDS_HEADS" not in _SRC            # one definition
    picks = re.findall(r"if \(H <= (\d+)u\) ctj_body_lds<(\d+)>", _SRC)
    assert [(int(b), int(i)) for b, i in picks] == list(zip(CC.BOUNDARIES[:-1], CC.ITEMS[:-1]))
    assert "else ctj_body_lds<CTJ_ITEMS>" in _SRC and CC.ITEMS[-1] == CC.LDS_HEADS // 1024
    assert all(b == 1024 * i for b, i in zip(CC.BOUNDARIES, CC.ITEMS))          # thread tid owns heads tid + 1024 i, i < ITEMS


def test_head_count_of_small_masks_by_hand():
    # A pixel on its own: one head by definition, wherever it lies.
    for y, x in ((0, 0), (3, 5), (2, 4)):
        assert CC.head_count(_mask(6, 8, [(y, x)])) == 1
        assert CC.head_count(_mask(6, 8, [(y, x)]), sparse=True) == 1

    # 2x2 block, rows 2-3, columns 4-5.
    #  (2,4) neighbours E, SE, S; cracks W and N, both eligible (even row; column 4).  Clockwise from W: NW, N, NE are background, E is
    #        foreground; clockwise from N: NE, then E.  Both cracks are swept by the state (E): ONE head.
    #  (2,5) neighbours W, SW, S; cracks E (eligible: even row) and N (column 5: not).  Clockwise from E: SE, then S: one head.
    #  (3,4) neighbours N, NE, E; cracks W (odd row and N above: not eligible) and S (column 4: eligible): one head.
    #  (3,5) neighbours NW, N, W; cracks E (odd row, nothing above (3,6): not) and S (column 5: not): none.
    assert CC.head_count(_mask(6, 8, [(2, 4), (2, 5), (3, 4), (3, 5)])) == 3

    # 1 x 9 bar, columns 3-11.  A tip has one neighbour, so one state, which sweeps its three cracks; an inner pixel has its N crack
    # swept by the state (E) and its S crack by the state (W), eligible in columns 4 and 8 only: 2 + 2 heads.
    #  even row 2: left tip: the W crack is eligible: 1.  right tip (2,11): the E crack is eligible (even row): 1.  -> 6
    #  odd row 3:  left tip: nothing above it, so its W crack is eligible: 1.  right tip (3,11): E crack in an odd row with nothing
    #              above (3,12), N / S cracks in column 11: no eligible crack, no head.                                          -> 5
    bar = [(0, x) for x in range(3, 12)]
    assert CC.head_count(_mask(6, 16, [(2, x) for _, x in bar])) == 6
    assert CC.head_count(_mask(6, 16, [(3, x) for _, x in bar])) == 5
    # the sparse cut (rows y % 4, columns x % 8), row 2: left tip by "nothing above": 1; column 8: 2; right tip: none.           -> 3
    assert CC.head_count(_mask(6, 16, [(2, x) for _, x in bar]), sparse=True) == 3

    # 3x3 ring, rows 2-4, columns 4-6, hole at (3,5).
    #  (2,4) neighbours E, S; cracks W, N, both swept by the state (E), eligible: 1
    #  (2,5) neighbours W, E, SW, SE; cracks N, S in column 5: 0
    #  (2,6) neighbours W, S; cracks E (even row: eligible), N (column 6: not): 1
    #  (3,4) neighbours N, NE, SE, S; cracks W (odd row, N above: not) and E, whose background pixel (3,5) has (2,5) above it:
    #        eligible - the crack the hole border starts at: 1
    #  (3,6) neighbours NW, N, SW, S; cracks W (NW above: not), E (odd row, nothing above (3,7)): 0
    #  (4,4) neighbours N, E; cracks W (even row) and S (column 4), both swept by the state (N): 1
    #  (4,5) neighbours NW, NE, W, E; cracks N, S in column 5: 0
    #  (4,6) neighbours N, W; cracks E (even row: eligible; state (W)), S (column 6: not): 1
    ring = [(y, x) for y in (2, 3, 4) for x in (4, 5, 6) if (y, x) != (3, 5)]
    assert CC.head_count(_mask(7, 10, ring)) == 5


def test_worst_word_fits_a_byte():
    """k_ct_headmaps keeps a word's head count in a uint8_t (cnt8).  The checkerboard reaches the bound of 96 that the argument in
    contour_cases.densest_word gives; no mask of the builders and no noise comes near 256."""
    wh = CC.word_heads(CC.densest_word())
    assert wh[2, 1] == CC.DENSEST_WORD_HEADS == 96 and wh.max() == 96 < 256
    assert CC.word_heads(CC.densest_word(), sparse=True).max() <= 96
    rng = np.random.default_rng(2)
    worst = 0
    for p in (0.2, 0.35, 0.5, 0.65):
        worst = max(worst, int(CC.word_heads((rng.random((24, 192)) < p).astype(np.uint8) * 255).max()))
    for _ in range(4):
        worst = max(worst, int(CC.word_heads(CC.tiled_4x4(rng, 24, 192)).max()))
    assert 0 < worst <= 96
    for name, fam, H, shape in CC.boundary_cases():
        if H in (CC.BOUNDARIES[0], CC.BOUNDARIES[-1] + 1):
            assert CC.word_heads(CC.build(fam, H, shape)).max() <= 96, name


@pytest.mark.parametrize("name,fam,H,shape", CC.boundary_cases(), ids=[c[0] for c in CC.boundary_cases()])
def test_builders_give_exact_head_counts(oracle, name, fam, H, shape):
    m = CC.build(fam, H, shape)
    assert m.shape == shape and m.dtype == np.uint8 and set(np.unique(m)) <= {0, 255}
    hs = CC.heads(m)
    assert len(hs) == H
    assert CC.head_count(m, sparse=True) < H
    cs, holes = oracle.find_contours(m, oracle.RETR_LIST, oracle.CHAIN_APPROX_NONE, with_holes=True)
    lone = sum(1 for _, _, s in hs if s < 0)
    assert lone >= 4 and sum(1 for c in cs if len(c) == 1) == lone
    if fam == "snake":
        # one long cycle: the heads on the pixels of the oracle's longest border are at least half of all
        big = max(cs, key=len)
        on = {(int(y), int(x)) for x, y in big.reshape(-1, 2)}
        carried = sum(1 for y, x, _ in hs if (y, x) in on)
        assert carried >= (H + 1) // 2 and carried == H - lone
        assert not holes.any() and len(cs) == lone + 1
    else:
        # rings inside the holes of rings: the oracle's hole borders; RETR_EXTERNAL keeps the frame-wide ring, the cells below it and
        # nothing of what lies in its hole
        import contour_tree_restate as R
        assert holes.sum() >= 7
        ext = oracle.find_contours(m, oracle.RETR_EXTERNAL, oracle.CHAIN_APPROX_SIMPLE)
        assert 2 <= len(ext) < len(cs) // 4
        if H == CC.BOUNDARIES[0]:
            _, _, hier = R.topological(m, R.RETR_TREE)
            depth, deepest = {}, 0
            for i in range(len(hier)):                    # pre-order: a parent comes before its children
                depth[i] = 0 if hier[i, 3] < 0 else depth[int(hier[i, 3])] + 1
                deepest = max(deepest, depth[i])
            assert deepest == 7                           # ring, its hole, and three rings with their holes inside it


@pytest.mark.parametrize("N", [127, 128, 255, 256, 257])
def test_nests_with_a_chosen_number_of_borders(oracle, N):
    m = CC.nests_contours(N)
    cs, holes = oracle.find_contours(m, oracle.RETR_LIST, oracle.CHAIN_APPROX_SIMPLE, with_holes=True)
    assert len(cs) == N and holes.sum() >= 7 and m.shape[1] % 64 != 0
