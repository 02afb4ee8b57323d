"""CPU suite for the plan of the contour-geometry pass (csrc/vp_geometry_plan.h through vp_contour_geometry_plan) and for what the
entries refuse from their arguments alone, before a device is touched: negative counts and missing pointers (VP_ERR_INVALID), the
coordinate bound and the perimeter bound (VP_ERR_UNSUPPORTED)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, -1, -4


def _plan_text():
    return open(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc", "vp_geometry_plan.h")).read()


def _define(name):
    return int(re.search(r"#define %s (\d+)" % name, _plan_text()).group(1))


def _plan(nc, npts, hulls=0):
    from vision import _vp
    ws, grid, cap = C.c_uint64(0), (C.c_int32 * 3)(), C.c_int32(0)
    rc = _vp.lib().vp_contour_geometry_plan(nc, npts, hulls, C.byref(ws), grid, C.byref(cap))
    return rc, ws.value, list(grid), cap.value


def test_plan_numbers():
    cap, tb = _define("GEOM_HULL_CAP"), _define("GEOM_TB")
    assert tb == 64 and cap >= 64 and cap & (cap - 1) == 0, "one wave per contour; the sorting network needs a power of two"
    assert 2 * 4 * cap + 64 <= 64 * 1024, "two arrays of packed points per wave within a block's LDS"
    rc, ws, grid, got_cap = _plan(5, 1000)
    assert rc == OK and grid == [5, 1, tb] and got_cap == cap
    al = lambda n: (n + 255) // 256 * 256
    assert ws == al(5 * 64) + 4096 + al(1000 * 8) + al(5 * 8) + al(5 * 4)
    assert _plan(5, 1000, 1)[1] == ws + al(1000 * 8)
    assert _plan(0, 0)[0] == OK and _plan(0, 0)[2][0] == 0
    # launches depend on the counts only
    assert _plan(17, 1)[2] == _plan(17, 1 << 20)[2] == [17, 1, tb]


def test_plan_refusals_and_the_perimeter_bound():
    from vision import _vp
    text = _plan_text()
    assert "(1ll << 53)" in text and "2^53" in text and "(1ll << 23)" in text, "the bound of the integer perimeter is stated in the plan header"
    assert _plan(-1, 0)[0] == INVALID and _plan(1, -1)[0] == INVALID
    assert _plan(1, 1 << 23)[0] == OK
    assert _plan(1, (1 << 23) + 1)[0] == UNSUPPORTED                    # 2^23 segments below 2^40 units each: the 64-bit total cannot wrap below it
    assert b"2^53" in _vp.lib().vp_last_error(None)
    assert _plan(1 << 24, 0)[0] == OK and _plan((1 << 24) + 1, 0)[0] == UNSUPPORTED


def test_entries_refuse_from_their_arguments():
    from vision import _vp
    L = _vp.lib()
    rows = np.zeros(4, _vp.CONTOUR_GEOM_DTYPE)
    pts = np.array([[0, 0], [3, 0], [3, 4]], np.int32)
    counts = np.array([3], np.int32)
    # (the context is NULL throughout: every refusal below comes before it is looked at)
    assert L.vp_contour_geometry_i32(None, pts.ctypes.data, counts.ctypes.data, -1, rows.ctypes.data, None, None) == INVALID
    assert L.vp_contour_geometry_i32(None, pts.ctypes.data, np.array([-3], np.int32).ctypes.data, 1, rows.ctypes.data, None, None) == INVALID
    assert L.vp_contour_geometry_i32(None, None, counts.ctypes.data, 1, rows.ctypes.data, None, None) == INVALID
    assert L.vp_contour_geometry_i32(None, pts.ctypes.data, None, 1, rows.ctypes.data, None, None) == INVALID
    assert L.vp_contour_geometry_i32(None, pts.ctypes.data, counts.ctypes.data, 1, None, None, None) == INVALID
    for bad in (32768, -32769, 1 << 20):
        far = pts.copy()
        far[1, 1] = bad
        assert L.vp_contour_geometry_i32(None, far.ctypes.data, counts.ctypes.data, 1, rows.ctypes.data, None, None) == UNSUPPORTED, bad
        assert b"[-32768, 32767]" in L.vp_last_error(None)
        out = (C.c_float * 3)()
        assert L.vp_min_enclosing_circle_i32(far.ctypes.data, 3, out, None) == UNSUPPORTED
    edge = np.array([[-32768, 32767], [32767, -32768]], np.int32)
    out = (C.c_float * 3)()
    assert L.vp_min_enclosing_circle_i32(edge.ctypes.data, 2, out, None) == OK
    assert L.vp_min_enclosing_circle_i32(None, 2, out, None) == INVALID and L.vp_min_enclosing_circle_i32(edge.ctypes.data, -1, out, None) == INVALID
    assert L.vp_min_enclosing_circle_i32(edge.ctypes.data, 2, None, None) == INVALID
    # the device forms: pointers, alignment, frame count, capacities
    assert L.vp_contour_geometry_dev(None, None, 8, 8, 1, rows.ctypes.data, None) == INVALID
    assert L.vp_contour_geometry_dev(None, 8, None, 8, 1, rows.ctypes.data, None) == INVALID
    assert L.vp_contour_geometry_dev(None, 8, 8, 8, -1, rows.ctypes.data, None) == INVALID
    assert L.vp_contour_geometry_dev(None, 12, 8, 8, 1, rows.ctypes.data, None) == INVALID          # points not 8-byte aligned
    assert L.vp_contour_geometry_dev(None, 8, 8, 8, (1 << 24) + 1, rows.ctypes.data, None) == UNSUPPORTED
    cd = _vp.make_contour_desc(max_contours=4, max_points=64)
    cb = _vp.ContourBuffers()
    assert L.vp_contour_geometry_batch_dev(None, C.byref(cd), C.byref(cb), 1, rows.ctypes.data) == INVALID    # no buffers
    cb.info = cb.counts = cb.offsets = cb.points = 256
    assert L.vp_contour_geometry_batch_dev(None, None, C.byref(cb), 1, rows.ctypes.data) == INVALID
    assert L.vp_contour_geometry_batch_dev(None, C.byref(cd), C.byref(cb), 1, None) == INVALID
    assert L.vp_contour_geometry_batch_dev(None, C.byref(cd), C.byref(cb), 65536, rows.ctypes.data) == INVALID
    big = _vp.make_contour_desc(max_contours=4, max_points=(1 << 23) + 1)
    assert L.vp_contour_geometry_batch_dev(None, C.byref(big), C.byref(cb), 1, rows.ctypes.data) == UNSUPPORTED
    # a good call reaches the context check
    assert L.vp_contour_geometry_batch_dev(None, C.byref(cd), C.byref(cb), 1, rows.ctypes.data) == INVALID
    assert L.vp_contour_geometry_i32(None, pts.ctypes.data, counts.ctypes.data, 1, rows.ctypes.data, None, None) == INVALID
