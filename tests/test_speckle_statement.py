"""CPU suite for the speckle filter's statement: tests/speckle_restate.py on hand-made images with known answers, and
vp_filter_speckles_host (the same statement as scalar C++) equal to it on all of them and on seeded int16 noise."""
import numpy as np

import speckle_cases as SC
import speckle_restate as R

NV = -16


def _both(img, new_val, max_size, max_diff):
    img = np.asarray(img, np.int16)
    want = R.filter_speckles(img, new_val, max_size, max_diff)
    got = SC.host_filter(img, new_val, max_size, max_diff)
    assert got.dtype == np.int16 and np.array_equal(got, want), f"the host routine differs from the statement in {int((got != want).sum())} pixels"
    return want


def test_a_region_at_the_limit_goes_and_one_above_it_stays():
    img = np.full((5, 9), NV, np.int16)
    img[1, 1:4] = 40            # three pixels
    img[3, 1:5] = 40            # four
    out = _both(img, NV, 3, 0)
    assert np.all(out[1] == NV) and np.array_equal(out[3], img[3])
    assert np.array_equal(_both(img, NV, 2, 0), img)
    assert np.all(_both(img, NV, 4, 0) == NV)


def test_links_chain_along_a_ramp():
    ramp = np.arange(12, dtype=np.int16)[None, :] * np.ones((1, 1), np.int16)
    assert np.array_equal(_both(ramp, NV, 11, 1), ramp)                 # one region of 12
    assert np.all(_both(ramp, NV, 12, 1) == NV)
    assert np.all(_both(ramp, NV, 1, 0) == NV)                          # twelve regions of one
    assert np.array_equal(_both(ramp, NV, 0, 0), ramp)
    lab, sizes = R.regions(ramp, NV, 1)
    assert sizes.tolist() == [0, 12] and R.regions(ramp, NV, 0)[1].tolist() == [0] + [1] * 12
    # the step is compared with the neighbour, not with the seed: 0 and 11 are eleven apart
    assert lab[0, 0] == lab[0, 11]


def test_diagonal_neighbours_are_not_linked():
    img = np.full((4, 4), NV, np.int16)
    img[0, 0] = img[1, 1] = img[2, 2] = img[3, 3] = 9
    assert R.regions(img, NV, 0)[1].tolist() == [0, 1, 1, 1, 1]
    assert np.all(_both(img, NV, 1, 0) == NV)
    img[1, 0] = 9                                                        # (0,0)-(1,0)-(1,1) is now one region of three
    out = _both(img, NV, 2, 0)
    assert out[0, 0] == out[1, 0] == out[1, 1] == 9 and out[2, 2] == NV and out[3, 3] == NV


def test_new_val_separates_regions_and_is_never_counted():
    img = np.full((1, 9), 30, np.int16)
    img[0, 4] = NV                                                       # two regions of four
    assert R.regions(img, NV, 0)[1].tolist() == [0, 4, 4]
    assert np.all(_both(img, NV, 4, 0) == NV)
    assert np.array_equal(_both(img, NV, 3, 0), img)
    img[0, 4] = NV + 1                                                   # not new_val: links both at max_diff 100
    assert R.regions(img, NV, 100)[1].tolist() == [0, 9]


def test_new_val_may_lie_inside_the_range_of_real_values():
    img = np.array([[7, 8, 9, 8, 7], [7, 8, 8, 8, 7]], np.int16)
    # with new_val 8 the 8s are nobody's: left 7s, right 7s and the lone 9 remain
    lab, sizes = R.regions(img, 8, 1)
    assert sizes.tolist() == [0, 2, 1, 2]
    out = _both(img, 8, 1, 1)
    assert out.tolist() == [[7, 8, 8, 8, 7], [7, 8, 8, 8, 7]]
    assert np.all(_both(img, 8, 2, 1) == 8)


def test_max_speckle_size_zero_copies():
    img = SC.noise(9, 14, (7, 8, 20), 1, holes=0.1)
    assert np.array_equal(_both(img, NV, 0, 0), img)
    assert np.all(_both(img, NV, img.size, 65535) == NV)                 # everything is a speckle


def test_differences_are_taken_in_int32():
    img = np.array([[32767, -32768, 32767, -32767]], np.int16)
    assert R.regions(img, 0, 65534)[1].tolist() == [0, 1, 1, 2]
    assert R.regions(img, 0, 65535)[1].tolist() == [0, 4]
    _both(img, 0, 1, 65534)
    _both(img, 0, 1, 65535)


def test_host_routine_equals_the_statement_on_noise_and_on_the_gpu_cases():
    rng = np.random.default_rng(11)
    full = rng.integers(-32768, 32768, (23, 31)).astype(np.int16)
    for md in (0, 9000, 30000, 65535):
        for size in (1, 5, 40):
            _both(full, int(full[3, 3]), size, md)
    for case in SC.cases(SC.tile()):
        got = SC.host_filter(case["image"](), case["new_val"], case["max_size"], case["max_diff"])
        assert np.array_equal(got, SC.expected(case)), case["id"]


def test_host_routine_on_padded_rows_and_in_place():
    from vision import _vp
    img = SC.noise(11, 13, (7, 8, 20), 2, holes=0.1)
    want = R.filter_speckles(img, NV, 3, 0)
    src = np.full((11, 17), 99, np.int16)
    src[:, :13] = img
    dst = np.full((11, 19), 12345, np.int16)
    _vp.check(_vp.lib().vp_filter_speckles_host(src.ctypes.data, 34, 13, 11, NV, 3, 0, dst.ctypes.data, 38))
    assert np.array_equal(dst[:, :13], want) and np.all(dst[:, 13:] == 12345)
    _vp.check(_vp.lib().vp_filter_speckles_host(src.ctypes.data, 34, 13, 11, NV, 3, 0, src.ctypes.data, 34))      # dst == src, as cv2 filters
    assert np.array_equal(src[:, :13], want) and np.all(src[:, 13:] == 99)
