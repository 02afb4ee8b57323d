"""GPU suite for vp_reproject_to_3d_*: bit for bit against tests/rectify_restate.py over the reprojection cases of tests/rectify_cases.py
- int16 disparities with the invalid value, 0, +-1, 32767 and -32768, float32 disparities with NaN and the infinities, a Q whose W is 0
on one column, rows of 1, 3, 4 and 5 pixels, a rig's Q and a general one - on packed and padded device images, on host images and
through the Python layer.

The products and sums of Q (x, y, d, 1) carry no fused multiply-add on either side: the kernel and the host statement compile one
formula (vp_rectify_plan.h) with contraction off, and numpy never fuses; double division and the cast to float32 are correctly
rounded on both."""
import numpy as np
import pytest

import rectify_cases as RC
import rectify_restate as R

pytestmark = pytest.mark.gpu

CASES = RC.reproject_cases()
INT_MIN = -2 ** 31


def _dev_call(vp, disp, q, invalid, dpad=0, xpad=0):
    from vision.devmat import DeviceMat
    ctx = vp.default_context()
    h, w = disp.shape
    buf = np.full((h, w + dpad), 77, disp.dtype)
    buf[:, :w] = disp
    dd = DeviceMat.from_host(ctx, buf)
    dx = DeviceMat.from_host(ctx, np.full((h, 3 * w + xpad), 777.0, np.float32))
    vp.check(vp.lib().vp_reproject_to_3d_dev(ctx.handle, dd.dev_ptr, buf.strides[0], 0 if disp.dtype == np.int16 else 1, w, h, q.ctypes.data,
                                             INT_MIN if invalid is None else invalid, dx.dev_ptr, 4 * (3 * w + xpad)), ctx.handle)
    out = dx.host_copy()
    assert np.all(out[:, 3 * w:] == 777.0), "the padding was written"
    assert R.same_bits(dd.host_copy(), buf), "the disparity was written"
    return np.ascontiguousarray(out[:, :3 * w]).reshape(h, w, 3)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_every_entry_form_equals_the_statement(vp, case):
    from vision.devmat import DeviceMat
    from vision.utils import stereo
    disp, q, invalid = case["disp"], np.ascontiguousarray(case["Q"]), case["invalid"]
    want = R.reproject(disp, q, invalid)
    assert R.same_bits(_dev_call(vp, disp, q, invalid), want), "dev"
    assert R.same_bits(_dev_call(vp, disp, q, invalid, dpad=3, xpad=5), want), "padded"
    assert R.same_bits(_dev_call(vp, disp, q, invalid, dpad=4, xpad=8), want), "padded by quads"
    got = stereo.reproject_to_3d(disp, q, invalid)                                       # vp_reproject_to_3d_i16 / _f32
    assert isinstance(got, np.ndarray) and R.same_bits(got, want), "host images"
    dev = stereo.reproject_to_3d(DeviceMat.from_host(vp.default_context(), disp), q, invalid)
    assert isinstance(dev, DeviceMat) and dev.shape == disp.shape + (3,) and R.same_bits(dev.host_copy(), want), "Python layer, device image"


def test_facade_reads_the_values_as_pixels(vp):
    from vision import cv2_facade as f
    rng = np.random.default_rng(5)
    d16 = rng.integers(-16, 600, (7, 9)).astype(np.int16)
    want = R.reproject(d16.astype(np.float32), RC.Q_GENERAL)
    assert R.same_bits(f.reprojectImageTo3D(d16, RC.Q_GENERAL), want)
    assert R.same_bits(f.reprojectImageTo3D(d16.astype(np.float32), RC.Q_GENERAL, ddepth=f.CV_32F), want)
    out = np.zeros((7, 9, 3), np.float32)
    assert f.reprojectImageTo3D(d16.astype(np.float32)[:, :, None], RC.Q_GENERAL, out) is out and R.same_bits(out, want)
