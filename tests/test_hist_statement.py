"""CPU suite for tests/hist_restate.py, the statement the GPU suite compares against: every case here is small enough to work out on
paper, and the expected values below were."""
import math

import numpy as np
import pytest

import hist_restate as R

CH0 = np.array([[0, 1, 2, 3], [4, 0, 1, 2], [3, 3, 0, 9], [1, 1, 2, 2]], np.uint8)
CH1 = np.array([[8, 15, 16, 23], [8, 24, 7, 16], [8, 16, 8, 8], [23, 24, 15, 7]], np.uint8)
IMG = np.stack([CH0, CH1], axis=2)
# channel 0 over [0, 4) in 2 bins: 0, 1 -> 0; 2, 3 -> 1; 4 and 9 -> none.  channel 1 over [8, 24) in 2 bins: 8..15 -> 0; 16..23 -> 1;
# 7 and 24 -> none
SIZES, RANGES = (2, 2), (0, 4, 8, 24)


def nine():
    """a 9 x 9 image with weights 1 and 3 on the diagonal"""
    p = np.zeros((9, 9), np.uint8)
    p[3, 3], p[4, 4] = 1, 3
    return p


def test_a_4x4_two_channel_image_with_ranges_that_exclude_values():
    bins = R.pixel_bins(IMG, (0, 1), SIZES, RANGES)
    assert bins.tolist() == [[0, 0, 3, 3], [-1, -1, -1, 3], [2, 3, 0, -1], [1, -1, 2, -1]]
    got = R.calc_hist(IMG, (0, 1), SIZES, RANGES)
    assert got.dtype == np.float32 and got.tolist() == [[3, 1], [2, 4]] and got.sum() == 10
    mask = np.ones((4, 4), np.uint8)
    mask[0] = 0
    assert R.calc_hist(IMG, (0, 1), SIZES, RANGES, mask).tolist() == [[1, 1], [2, 2]]
    mask[:] = 0
    assert R.calc_hist(IMG, (0, 1), SIZES, RANGES, mask).sum() == 0
    # one dimension over the second channel, and the dimensions the other way round
    assert R.calc_hist(IMG, (1,), (2,), (8, 24)).tolist() == [7, 5]              # 24, 7, 24 and 7 fall outside
    assert R.calc_hist(IMG, (1, 0), SIZES, (8, 24, 0, 4)).tolist() == [[3, 2], [1, 4]]
    assert R.calc_hist_counts(IMG, (0, 1), SIZES, RANGES).dtype == np.uint32


def test_a_value_on_a_bin_edge_and_on_the_exclusive_upper_end():
    t = R.bin_tables((2,), (8, 24))[0]
    assert [t[j] for j in (7, 8, 15, 16, 23, 24, 255)] == [-1, 0, 0, 1, 1, -1, -1]
    hue = R.bin_tables((180,), (0, 180))[0]
    assert hue[0] == 0 and hue[179] == 179 and hue[180] == -1 and (hue[:180] == np.arange(180)).all()
    full = R.bin_tables((256,), (0, 256))[0]
    assert (full == np.arange(256)).all()
    # [10.5, 200.25) in 7 bins of 27.107...: bin k starts at 10.5 + 27.107 k
    odd = R.bin_tables((7,), (10.5, 200.25))[0]
    assert [odd[j] for j in (10, 11, 37, 38, 64, 65, 200, 201)] == [-1, 0, 0, 1, 1, 2, 6, -1]
    one = R.bin_tables((1,), (100, 101))[0]
    assert one[99] == -1 and one[100] == 0 and one[101] == -1


def test_ties_round_to_even_and_products_saturate():
    hist = np.array([1, 3, 5, 7, 600, -3, 0], np.float32)
    assert R.fold(hist, 0.5).tolist() == [0, 2, 2, 4, 255, 0, 0]          # 0.5 1.5 2.5 3.5 300 -1.5 0
    assert R.fold(np.array([509, 510, 511], np.float32), 0.5).tolist() == [254, 255, 255]      # 254.5 -> 254, 255, 255.5 -> 255
    assert R.fold(np.array([np.nan, np.inf, -np.inf], np.float32), 1.0).tolist() == [0, 255, 0]
    got = R.back_project(IMG, (0, 1), np.array([[3, 1], [2, 4]], np.float32), RANGES, 0.5)      # the table: [[2, 0], [1, 2]]
    assert got.dtype == np.uint8 and got.tolist() == [[2, 2, 2, 2], [0, 0, 0, 2], [1, 2, 2, 0], [0, 0, 1, 0]]
    assert R.back_project(IMG, (0, 1), np.array([[3, 1], [2, 4]], np.float32), RANGES, 100).tolist() == \
        [[255, 255, 255, 255], [0, 0, 0, 255], [200, 255, 255, 0], [100, 0, 200, 0]]


def test_normalize_is_one_rounding_of_the_double_stretch():
    got = R.normalize_hist(np.array([2, 4, 3, 10], np.float32), 255)
    assert got.dtype == np.float32 and got.tolist() == [0.0, 63.75, 31.875, 255.0]
    assert R.normalize_hist(np.array([5, 5], np.float32)).tolist() == [0.0, 0.0]
    third = R.normalize_hist(np.array([0, 1, 3], np.float32), 1.0)
    assert third[1] == np.float32(1.0 / 3.0)


def test_a_mean_shift_run_of_three_iterations_on_a_9x9_image():
    """window 4 x 4 from (0, 0), half a side 2.0.  Iteration 0: only the 1 at (3, 3), centroid (3, 3), step (+1, +1), squared 2.
    Iteration 1 at (1, 1): the 1 at relative 2 and the 3 at relative 3, centroid 11 / 4 = 2.75, step round(0.75) = +1 each way.
    Iteration 2 at (2, 2): relative 1 and 2, centroid 7 / 4 = 1.75, step round(-0.25) = 0: the squared step 0 is below eps2 = 1."""
    p = nine()
    assert R.window_sums(p, (0, 0, 4, 4)) == (1, 3, 3) == R.window_sums_fast(p, (0, 0, 4, 4))
    assert R.window_sums(p, (1, 1, 4, 4)) == (4, 11, 11) and R.window_sums(p, (2, 2, 4, 4)) == (4, 7, 7)
    assert R.mean_shift(p, (0, 0, 4, 4), 10, 1.0) == (2, (2, 2, 4, 4))
    assert R.mean_shift(p, (0, 0, 4, 4)) == (2, (2, 2, 4, 4))                  # no criteria: 100 iterations, eps2 = 1
    assert R.mean_shift(p, (0, 0, 4, 4), 2, 1.0) == (2, (2, 2, 4, 4))          # stopped by the count, same place
    assert R.mean_shift(p, (0, 0, 4, 4), 1, 1.0) == (1, (1, 1, 4, 4))
    assert R.mean_shift(p, (0, 0, 4, 4), 0, 1.0) == (1, (1, 1, 4, 4))          # max(max_iter, 1)
    assert R.mean_shift(p, (0, 0, 4, 4), 10, 2.0) == (0, (1, 1, 4, 4))         # eps2 = 4 > 2: stops in the first iteration, after the move
    assert R.mean_shift(p, (0, 0, 4, 4), 10, -3.0) == (10, (2, 2, 4, 4))       # eps2 = 0: no step is below it
    assert R.criteria(5, 1.5) == (5, 2) and R.criteria(5, 2.5) == (5, 6) and R.criteria(None, None) == (100, 1)      # 2.25 -> 2, 6.25 -> 6


def test_a_window_that_leaves_the_image():
    p = nine()
    assert R.intersect((-2, -2, 6, 6), 9, 9) == (0, 0, 4, 4) and R.intersect((7, 8, 5, 5), 9, 9) == (7, 8, 2, 1)
    assert R.intersect((9, 0, 3, 3), 9, 9) == (0, 0, 0, 0) == R.intersect((-3, 0, 3, 3), 9, 9)
    assert R.mean_shift(p, (-2, -2, 6, 6), 10, 1.0) == (2, (2, 2, 4, 4))       # W is the part inside: the run above
    for bad in ((9, 9, 2, 2), (-5, 0, 5, 5), (0, 0, 0, 3), (0, 0, 3, -1)):
        with pytest.raises(ValueError):
            R.mean_shift(p, bad, 10, 1.0)
    # inside the loop a window outside the image is re-centred at (cols / 2, rows / 2) with sides of 1: the 3 at (4, 4) has centroid
    # 0, the step is round(0 - 2.0) = -2 each way
    assert R.mean_shift_loop(p, (20, 20, 4, 4), (0, 0, 4, 4), 1, 1) == ((2, 2, 1, 1), 1)
    # a step is clamped into the image: all the mass in the last column of a window at the right edge
    q = np.zeros((9, 9), np.uint8)
    q[0:4, 8] = 7
    assert R.mean_shift(q, (5, 0, 4, 4), 10, 1.0) == (0, (5, 0, 4, 4))         # centroid x 3 -> +1, clamped to 0; y 1.5 - 2 -> -0 -> 0


def test_no_mass_stops_at_once():
    z = np.zeros((9, 9), np.uint8)
    assert R.mean_shift(z, (2, 3, 4, 5), 10, 1.0) == (0, (2, 3, 4, 5))
    p = nine()
    assert R.mean_shift(p, (5, 5, 4, 4), 10, 1.0) == (0, (5, 5, 4, 4))         # the mass lies outside the window


def test_camshift_finish_by_hand():
    assert R.grow((3, 25, 10, 4), 30, 30) == (0, 15, 30, 15) and R.grow((12, 12, 4, 4), 30, 30) == (2, 2, 24, 24)
    # one pixel of 5 at (15, 12), the grown window at (5, 2): no spread, a box of no size around the pixel
    p = np.zeros((30, 30), np.uint8)
    p[12, 15] = 5
    assert R.raster_sums(p, (5, 2, 20, 20)) == (5, 50, 50, 500, 500, 500)
    box, win = R.cam_shift_finish((5, 50, 50, 500, 500, 500), (5, 2, 20, 20), 30, 30)
    assert win == (14, 11, 2, 2) and box == ((15.0, 12.0), (0.0, 0.0), 90.0)
    # a horizontal bar of ten ones: mu20 = 82.5, mu11 = mu02 = 0, theta = 0, length = 4 sqrt(8.25), width = 0
    bar = np.zeros((30, 30), np.uint8)
    bar[15, 10:20] = 1
    sums = R.raster_sums(bar, (0, 0, 30, 30))
    assert sums == (10, 145, 150, 2185, 2175, 2250)
    box, win = R.cam_shift_finish(sums, (0, 0, 30, 30), 30, 30)
    assert win == (8, 14, 13, 2)                                           # xc = round(14.5) = 14, 13 = round(11.49) + 2
    assert box == ((14.5, 15.0), (0.0, float(np.float32(math.sqrt(8.25) * 4))), 90.0)
    # a vertical bar: the axes swap, the angle turns by 90 degrees and folds into [0, 180)
    box, win = R.cam_shift_finish(R.raster_sums(bar.T.copy(), (0, 0, 30, 30)), (0, 0, 30, 30), 30, 30)
    assert win == (14, 8, 2, 13) and box == ((15.0, 14.5), (0.0, float(np.float32(math.sqrt(8.25) * 4))), 0.0)
    # no mass: the empty box and the window as it was grown
    assert R.cam_shift_finish((0, 0, 0, 0, 0, 0), (1, 2, 3, 4), 30, 30) == (((0.0, 0.0), (0.0, 0.0), 0.0), (1, 2, 3, 4))
    assert R.cam_shift(np.zeros((30, 30), np.uint8), (12, 12, 4, 4), 10, 1.0) == (((0.0, 0.0), (0.0, 0.0), 0.0), (2, 2, 24, 24))
