"""CPU suite: the standard Hough transform (cv2.HoughLines, utils/feature.py:183-213) as the tests state it (hough_restate.py), checked
against geometry; the mirror's and the facade's interface; no fallback to the statement when there is no GPU."""
import inspect
import math

import numpy as np
import pytest

import hough_restate as HR

STEP = np.pi / 180


def _brute(img, rho, theta, min_theta=0.0, max_theta=HR.CV_PI):
    """The accumulator by the C++ loop order, one float32 scalar operation at a time (checks the vectorised statement)."""
    h, w = img.shape
    rho_f, theta_f, irho, numrho, numangle = HR.geometry(w, h, rho, theta, min_theta, max_theta)
    tab_sin, tab_cos = HR.trig_tables(numangle, min_theta, theta_f, irho)
    acc = np.zeros((numangle + 2) * (numrho + 2), np.int64)
    for i in range(h):
        for j in range(w):
            if img[i, j]:
                for n in range(numangle):
                    v = np.float32(np.float32(j) * tab_cos[n]) + np.float32(np.float32(i) * tab_sin[n])
                    r = int(np.rint(np.float32(v))) + (numrho - 1) // 2
                    acc[(n + 1) * (numrho + 2) + r + 1] += 1
    return acc.reshape(numangle + 2, numrho + 2)


def test_statement_equals_the_scalar_loop():
    rng = np.random.default_rng(0)
    img = (rng.random((23, 31)) < 0.1).astype(np.uint8) * 255
    for rho, theta in ((1, STEP), (0.5, np.pi / 90), (3, 0.3)):
        acc, _ = HR.accumulator(img, rho, theta)
        assert np.array_equal(acc, _brute(img, rho, theta)), (rho, theta)


def test_full_row():
    img = np.zeros((160, 200), np.uint8)
    img[100, :] = 255
    acc, (_, _, numrho, numangle) = HR.accumulator(img, 1, STEP)
    assert numangle == 180
    lines = HR.hough_lines(img, 1, STEP, 150)
    assert lines.shape[1:] == (1, 2) and lines.dtype == np.float32
    rho, theta = lines[0, 0]
    assert rho == 100 and abs(theta - np.pi / 2) < 1e-6
    base, votes = HR.peaks(acc, 150)
    top = base[np.argmax(votes)]
    assert top // (numrho + 2) - 1 == 90 and votes.max() == 200


def test_full_column():
    img = np.zeros((120, 90), np.uint8)
    img[:, 50] = 1
    lines = HR.hough_lines(img, 1, STEP, 100)
    rho, theta = lines[0, 0]
    assert rho == 50 and theta == 0
    acc, (_, _, numrho, _) = HR.accumulator(img, 1, STEP)
    assert acc[1, 50 + (numrho - 1) // 2 + 1] == 120


def test_diagonal():
    img = np.zeros((150, 150), np.uint8)
    img[np.arange(150), np.arange(150)] = 255
    acc, (_, _, numrho, _) = HR.accumulator(img, 1, STEP)
    lines = HR.hough_lines(img, 1, STEP, 100)
    rho, theta = lines[0, 0]
    assert rho == 0 and abs(theta - 3 * np.pi / 4) < 1e-6
    assert acc[136, (numrho - 1) // 2 + 1] == 150


def test_empty_image():
    assert HR.hough_lines(np.zeros((40, 50), np.uint8), 1, STEP, 0) is None


def test_equal_peaks_come_lower_cell_first():
    img = np.zeros((160, 200), np.uint8)
    img[100, :] = 255
    img[40, :] = 255
    lines = HR.hough_lines(img, 1, STEP, 150)
    assert lines[0, 0, 0] == 40 and lines[1, 0, 0] == 100
    assert lines[0, 0, 1] == lines[1, 0, 1]


@pytest.mark.parametrize("theta,expect", [(np.pi / 180, 180), (np.pi / 360, 360), (0.3, 10), (1.0, 3), (2 * np.pi, 1), (0.7, 4)])
def test_number_of_angles(theta, expect):
    _, _, _, _, numangle = HR.geometry(100, 100, 1, theta)
    assert numangle == expect
    # the rule itself, in double on the float step
    t = float(np.float32(theta))
    n = math.floor(np.pi / t) + 1
    if n > 1 and abs(np.pi - (n - 1) * t) < t / 2:
        n -= 1
    assert numangle == n


def test_number_of_rho_cells():
    assert HR.geometry(640, 480, 1, STEP)[3] == 2 * 1120 + 1
    assert HR.geometry(640, 480, 0.5, STEP)[3] == 2 * (2 * 1120 + 1)
    assert HR.geometry(1920, 1080, 1, STEP)[3] + 2 == 6003
    assert HR.geometry(3, 2, 4, STEP)[3] == 3                    # cvRound(11 / 4.f)
    assert HR.geometry(3, 2, 22, STEP)[3] == 0                   # cvRound(0.5) = 0: no row of cells, no line
    assert HR.hough_lines(np.full((2, 3), 255, np.uint8), 22, STEP, 0) is None


def test_angle_range():
    img = np.zeros((160, 200), np.uint8)
    img[100, :] = 255
    lo, hi = np.pi / 4, 3 * np.pi / 4
    _, _, _, _, numangle = HR.geometry(200, 160, 1, STEP, lo, hi)
    assert numangle == HR.num_angle(lo, hi, float(np.float32(STEP))) == 91
    lines = HR.hough_lines(img, 1, STEP, 150, lo, hi)
    rho, theta = lines[0, 0]
    assert rho == 100 and abs(theta - np.pi / 2) < 1e-6
    assert np.all(lines[:, 0, 1] >= np.float32(lo)) and np.all(lines[:, 0, 1] <= np.float32(hi) + 1e-6)


def test_facade_signature_and_multiscale_refusal():
    from vision import cv2_facade
    names = list(inspect.signature(cv2_facade.HoughLines).parameters)
    assert names == ["image", "rho", "theta", "threshold", "lines", "srn", "stn", "min_theta", "max_theta"]
    assert inspect.signature(cv2_facade.HoughLines).parameters["max_theta"].default == cv2_facade.CV_PI == math.pi
    img = np.zeros((8, 8), np.uint8)
    with pytest.raises(cv2_facade.error):
        cv2_facade.HoughLines(img, 1, STEP, 10, None, 2, 0)
    with pytest.raises(cv2_facade.error):
        cv2_facade.HoughLines(img, 1, STEP, 10, None, 0, 3)
    with pytest.raises(cv2_facade.error):
        cv2_facade.HoughLines(img, 0, STEP, 10)
    with pytest.raises(cv2_facade.error):
        cv2_facade.HoughLines(img, 1, STEP, 10, None, 0, 0, 1.0, 0.5)


def test_line_polar_to_cartesian():
    from vision.utils.feature import line_polar_to_cartesian
    rng = np.random.default_rng(3)
    for rho, theta in [(np.float32(100), np.float32(np.pi / 2)), (np.float32(-37.5), np.float32(2.3))] + \
            [(np.float32(r), np.float32(t)) for r, t in zip(rng.uniform(-900, 900, 50), rng.uniform(0, np.pi, 50))]:
        a = np.cos(theta)
        b = np.sin(theta)
        x0 = a * rho
        y0 = b * rho
        ref = (int(x0 + 1000 * (-b)), int(y0 + 1000 * a), int(x0 - 1000 * (-b)), int(y0 - 1000 * a))
        got = line_polar_to_cartesian(rho, theta)
        assert got == ref and all(type(v) is int for v in got)


def test_no_fallback_to_the_statement():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu suite")
    from vision import _vp
    from vision.utils import feature
    img = np.zeros((32, 32), np.uint8)
    img[10, :] = 255
    with pytest.raises(_vp.VpError):
        feature.find_lines(img, 1, STEP, 10)
    n = _vp.C.c_int(-7)
    out = np.zeros(8, np.float32)
    assert _vp.lib().vp_hough_lines_u8(None, _vp.ptr(img), 32, 32, 1.0, STEP, 10, 0.0, np.pi, _vp.ptr(out), 4, _vp.C.byref(n)) == -1
    assert n.value == -7


def test_outside_path_names_still_raise():
    from vision.utils import feature
    for name in ("find_line_segments", "find_circles", "find_corners"):
        with pytest.raises(NotImplementedError):
            getattr(feature, name)(np.zeros((4, 4), np.uint8))
