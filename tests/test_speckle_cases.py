"""CPU suite: the cases of tests/speckle_cases.py cover what they claim, at the tile size the plan reports today - so that a later
change of the tile does not hollow them out silently."""
import numpy as np

import speckle_cases as SC
import speckle_restate as R

T = SC.tile()
CASES = {c["id"]: c for c in SC.cases(T)}


def _tiles(ys, xs):
    return {(int(y) // T, int(x) // T) for y, x in zip(ys, xs)}


def test_the_sizes_straddle_the_tile():
    assert {"size_1x1", "size_1x37", "size_37x1", f"size_{T}x{T}", f"size_{T + 1}x{T + 1}", f"size_{2 * T + 1}x{T - 1}"} <= set(CASES)
    assert SC.lib_plan(T, T)["grid"] == (1, 1) and SC.lib_plan(T + 1, T + 1)["grid"] == (2, 2) and SC.lib_plan(2 * T + 1, T - 1)["grid"] == (3, 1)
    for cid in (f"size_{T}x{T}", f"size_{T + 1}x{T + 1}", f"size_{2 * T + 1}x{T - 1}"):
        img = CASES[cid]["image"]()
        want = SC.expected(CASES[cid])
        assert np.any(want != img) and np.any((want == img) & (img != CASES[cid]["new_val"])), cid     # something goes, something stays


def test_the_serpentine_is_one_region_across_every_tile_edge():
    c = CASES["serpentine_at"]
    img = c["image"]()
    h, w = img.shape
    assert (w, h) == (3 * T + 1, 2 * T + 1) and SC.lib_plan(w, h)["grid"] == (4, 3)
    lab, sizes = R.regions(img, c["new_val"], c["max_diff"])
    path = lab[0, 0]
    assert np.all(lab[img == 100] == path) and sizes[path] == int((img == 100).sum()) == c["max_size"] == CASES["serpentine_below"]["max_size"] + 1
    ys, xs = np.nonzero(lab == path)
    assert len(_tiles(ys, xs)) == 12                                                            # it visits every tile
    # one pixel wide: no 2 x 2 block of path pixels
    p = img == 100
    assert not np.any(p[:-1, :-1] & p[1:, :-1] & p[:-1, 1:] & p[1:, 1:])
    # it crosses every vertical tile edge on its rows and every horizontal tile edge on a connector
    for k in range(1, 4):
        assert p[0, k * T - 1] and p[0, k * T]
    for k in range(1, 3):
        assert np.any(p[k * T - 1, :] & p[k * T, :])
    assert np.all(SC.expected(c)[p] == c["new_val"]) and np.all(SC.expected(CASES["serpentine_below"])[p] == 100)
    # the gaps between its rows are regions of their own, below the limit in both cases
    assert np.all(SC.expected(CASES["serpentine_below"])[~p] == c["new_val"])


def test_the_constant_image_is_one_region_and_the_empty_one_none():
    c = CASES["constant_kept"]
    img = c["image"]()
    assert R.regions(img, c["new_val"], c["max_diff"])[1].tolist() == [0, img.size] and img.shape == (2 * T + 1, 3 * T + 1)
    assert np.array_equal(SC.expected(c), img) and np.all(SC.expected(CASES["constant_removed"]) == -16)
    e = CASES["all_new_val"]
    assert R.regions(e["image"](), e["new_val"], e["max_diff"])[1].tolist() == [0] and np.all(SC.expected(e) == -16)


def test_the_ring_closes_around_a_tile_corner():
    c = CASES["ring_kept"]
    img = c["image"]()
    lab, sizes = R.regions(img, c["new_val"], c["max_diff"])
    ys, xs = np.nonzero(img == 7)
    assert len(ys) == 12 and len(set(lab[ys, xs])) == 1 and sizes[lab[ys[0], xs[0]]] == 12
    assert _tiles(ys, xs) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    inside = lab[T, T]
    assert sizes[inside] == 4 and inside != lab[0, 0]                                          # the ring is closed: its inside is cut off
    assert c["max_size"] == 11 and CASES["ring_removed"]["max_size"] == 12
    assert np.all(SC.expected(c)[ys, xs] == 7) and np.all(SC.expected(CASES["ring_removed"])[ys, xs] == -16)


def test_the_straddlers_cross_a_tile_edge_on_both_sides_of_the_limit():
    c = CASES["straddlers"]
    img = c["image"]()
    lab, sizes = R.regions(img, c["new_val"], c["max_diff"])
    bars = [n for n in range(1, len(sizes)) if np.all(img[lab == n] == 5)]
    assert sorted(sizes[bars].tolist()) == [6, 6, 7, 7] and c["max_size"] == 6
    for n in bars:
        ys, xs = np.nonzero(lab == n)
        assert len(_tiles(ys, xs)) == 2, "a bar lies inside one tile"
    want = SC.expected(c)
    for n in bars:
        assert np.all(want[lab == n] == (5 if sizes[n] == 7 else -16))
    across = {tuple(sorted(_tiles(*np.nonzero(lab == n)))) for n in bars}
    assert {((0, 0), (0, 1)), ((0, 0), (1, 0))} == across                                       # a vertical and a horizontal edge


def test_the_noise_holds_regions_on_both_sides_of_the_limit():
    sizes0 = R.regions(CASES["noise_diff0"]["image"](), -16, 0)[1][1:]
    sizes1 = R.regions(CASES["noise_diff1"]["image"](), -16, 1)[1][1:]
    for sizes in (sizes0, sizes1):
        assert (sizes == 4).any() and (sizes == 5).any() and (sizes <= 4).sum() > 20 and (sizes > 4).sum() > 5
    assert sizes1.max() > sizes0.max() and len(sizes1) < len(sizes0)                           # 7 and 8 join at max_diff 1
    assert not np.array_equal(SC.expected(CASES["noise_diff0"]), SC.expected(CASES["noise_diff1"]))
    c = CASES["new_val_inside"]
    img = c["image"]()
    assert img.min() < c["new_val"] < img.max() and np.any(SC.expected(c) != img) and np.all(SC.expected(c)[img == 8] == 8)
    a, b = CASES["extremes_65534"], CASES["extremes_65535"]
    assert len(R.regions(b["image"](), 0, 65535)[1]) == 2 and len(R.regions(a["image"](), 0, 65534)[1]) > 2
    assert not np.array_equal(SC.expected(a), SC.expected(b))
