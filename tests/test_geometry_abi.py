"""CPU suite for the surface of the contour geometry: the five C entries are exported by libvp.so and declared in include/vp.h with the
prototypes vision/_vp.py binds; both units are built; the row struct is 80 bytes and mirrored field for field by the ctypes Structure
and the numpy record; the status bits agree between header, plan and binding; vision.utils.feature and the facade have the names."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from abi_header import _header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vp_contour_geometry_i32", "vp_contour_geometry_dev", "vp_contour_geometry_batch_dev", "vp_contour_geometry_plan", "vp_min_enclosing_circle_i32"]


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_geometry_symbols_are_exported_declared_and_bound_alike():
    from vision import _vp
    protos = _header_prototypes()
    lib = C.CDLL(_vp.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name) and name in protos and name in _vp._SIGS, name
        assert protos[name][1] == list(_vp._SIGS[name][1]) and protos[name][0] == "int", name
    assert [len(protos[n][1]) for n in NEW] == [7, 7, 5, 6, 4]
    built = _read("cuauv-vision-pipeline_amd", "build.py")
    for src in ("vp_geometry.hip", "vp_api_geometry.hip"):
        assert f'"{src}"' in built, f"{src} is not among VP_SOURCES"
        assert os.path.exists(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc", src))
    assert os.path.exists(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc", "vp_geometry_plan.h"))


def test_row_struct_is_mirrored():
    from vision import _vp
    header = _read("include", "vp.h")
    body = re.search(r"typedef struct vp_contour_geom \{(.*?)\} vp_contour_geom;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(double|float|int64_t|int32_t|uint32_t|int16_t)\s+(\w+)(?:\[(\d+)\])?;", body)
    ctype = {"double": C.c_double, "float": C.c_float, "int64_t": C.c_int64, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int16_t": C.c_int16}
    want = [(name, ctype[t] * int(n) if n else ctype[t]) for t, name, n in fields]
    assert len(want) == 9 and _vp.ContourGeom._fields_ == want
    assert C.sizeof(_vp.ContourGeom) == 80 == _vp.CONTOUR_GEOM_DTYPE.itemsize
    for name, _ in want:
        assert getattr(_vp.ContourGeom, name).offset == _vp.CONTOUR_GEOM_DTYPE.fields[name][1], name
    assert "static_assert(sizeof(vp_contour_geom) == 80" in _read("cuauv-vision-pipeline_amd", "csrc", "vp_api_geometry.hip")
    assert "static_assert(sizeof(vp_geom_raw) == 64" in _read("cuauv-vision-pipeline_amd", "csrc", "vp_api_geometry.hip")


def test_status_bits_and_bounds_agree():
    from vision import _vp
    header, plan = _read("include", "vp.h"), _read("cuauv-vision-pipeline_amd", "csrc", "vp_geometry_plan.h")
    hv = {n: int(v) for n, v in re.findall(r"VP_GEOM_([A-Z_]+)\s*=\s*(\d+)", header)}
    pv = {n: int(v) for n, v in re.findall(r"#define GEOM_ST_([A-Z_]+)\s+(\d+)u", plan)}
    assert hv == pv == {"OK": 0, "HULL_CAP": 1, "PERIMETER": 2, "SKIPPED": 4, "COORD": 8}
    assert hv == {n[5:]: getattr(_vp, n) for n in dir(_vp) if n.startswith("GEOM_") and n[5:] in hv}
    assert int(re.search(r"#define GEOM_COORD_MIN \((-\d+)\)", plan).group(1)) == _vp.GEOM_COORD_MIN == -32768
    assert int(re.search(r"#define GEOM_COORD_MAX (\d+)", plan).group(1)) == _vp.GEOM_COORD_MAX == 32767


def test_python_names_and_signatures():
    from vision import cv2_facade as f
    from vision.utils import feature
    sig = lambda fn: [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(feature.contour_geometry) == [("contours", E), ("hulls", False)]
    assert sig(feature.min_enclosing_circle) == [("contour", E)] and sig(f.minEnclosingCircle) == [("points", E)]
    assert sig(feature.min_enclosing_rects) == [("contours", E)] and sig(feature.contour_perimeters) == [("contours", E), ("closed", True)]
    assert feature.GEOMETRY_DTYPE.names == ("perimeter", "perimeter_open", "hull_count", "hull_area", "rect", "circle", "status")
    assert feature.GEOMETRY_DTYPE["rect"].shape == (5,) and feature.GEOMETRY_DTYPE["circle"].shape == (3,)
    # the three it leaves alone keep their parameters
    assert [n for n, _ in sig(f.minAreaRect)] == ["points"] and [n for n, _ in sig(f.arcLength)] == ["curve", "closed"]
    assert [n for n, _ in sig(f.convexHull)] == ["points", "hull", "clockwise", "returnPoints"]
