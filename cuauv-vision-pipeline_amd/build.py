"""Builds the native libraries of this package in-tree (hipcc cross-compiles gfx950 without a GPU).

  lib/libvp.so   HIP kernels + C ABI of include/vp.h (the hot path)
  lib/libcamera_message_framework.so   shared-memory seqlock IPC (C++, no GPU)
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

VP_SOURCES = ["vp_api.hip", "vp_api_color.hip", "vp_api_morph_chain.hip", "vp_api_shapes.hip", "vp_api_label.hip", "vp_api_filter.hip", "vp_api_moments.hip", "vp_api_corners.hip", "vp_api_dist.hip", "vp_api_kmeans.hip", "vp_api_match.hip", "vp_api_hist.hip", "vp_api_flow.hip", "vp_api_model.hip", "vp_api_features.hip", "vp_api_geometry.hip", "vp_geometry.hip", "vp_api_stereo.hip", "vp_stereo.hip", "vp_api_speckle.hip", "vp_speckle.hip", "vp_api_sgm.hip", "vp_sgm.hip", "vp_api_rectify.hip", "vp_rectify.hip", "vp_api_plane.hip", "vp_plane.hip", "vp_api_rigid.hip", "vp_rigid.hip", "vp_color.hip", "vp_morph.hip", "vp_fill.hip", "vp_ccl.hip", "vp_balance.hip", "vp_yolo.hip", "vp_filter.hip", "vp_feed.hip", "vp_post.hip", "vp_hough.hip", "vp_hough_circles.hip", "vp_whitebal.hip", "vp_adaptive.hip", "vp_elementwise.hip", "vp_median.hip", "vp_deriv.hip", "vp_clahe.hip", "vp_remap.hip", "vp_box.hip", "vp_pyr.hip", "vp_integral.hip", "vp_moments.hip", "vp_corners.hip", "vp_dist.hip", "vp_kmeans.hip", "vp_match.hip", "vp_hist.hip", "vp_flow.hip", "vp_model.hip", "vp_features.hip", "vp_tables.cpp"]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def source_digest():
    """sha256 over the sources libvp.so is built from (csrc/vp_* + include/vp.h): profiles/ evidence records it, bench.py
    only reports counter-derived traffic collected from the very sources it is running."""
    import hashlib
    h = hashlib.sha256()
    files = sorted(f for f in os.listdir(CSRC) if f.startswith("vp_"))
    for f in files:
        h.update(f.encode())
        h.update(open(os.path.join(CSRC, f), "rb").read())
    h.update(open(os.path.join(HERE, "..", "include", "vp.h"), "rb").read())
    return h.hexdigest()


def build_libvp(force=False, verbose=False):
    """One object per translation unit (compiled in parallel, rebuilt when the unit or any shared header changed), then one link."""
    from concurrent.futures import ThreadPoolExecutor
    os.makedirs(LIBDIR, exist_ok=True)
    objdir = os.path.join(LIBDIR, "obj")
    os.makedirs(objdir, exist_ok=True)
    out = os.path.join(LIBDIR, "libvp.so")
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.startswith("vp_") and (f.endswith(".h") or f.endswith(".inl"))]
    headers.append(os.path.join(HERE, "..", "include", "vp.h"))
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=off",
             "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-result"]
    jobs = []
    objs = []
    for s in VP_SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(objdir, os.path.splitext(s)[0] + ".o")
        objs.append(obj)
        if force or _stale(obj, [src] + headers):
            jobs.append([HIPCC] + flags + ["-x", "hip", "-c", src, "-o", obj])

    def _run(cmd):
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
    if jobs:
        with ThreadPoolExecutor(max(1, min(len(jobs), os.cpu_count() or 1))) as ex:
            list(ex.map(_run, jobs))
    if jobs or force or _stale(out, objs):
        _run([HIPCC, "-shared", "-fPIC", "--offload-arch=gfx950"] + objs + ["-o", out])
    return out


def build_libcmf(force=False, verbose=False):
    os.makedirs(LIBDIR, exist_ok=True)
    out = os.path.join(LIBDIR, "libcamera_message_framework.so")
    src = os.path.join(CSRC, "cmf.cpp")
    if not os.path.exists(src):
        return None
    deps = [src, os.path.join(HERE, "..", "include", "camera_message_framework_c.h")]
    if not force and not _stale(out, deps):
        return out
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", src, "-o", out, "-lpthread", "-lrt"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_libbalance(force=False, verbose=False):
    """libauv-color-balance.so: the reference's process_frame entry (color_balance.hpp:9-14) bound to libvp."""
    out = os.path.join(LIBDIR, "libauv-color-balance.so")
    src = os.path.join(CSRC, "color_balance_shim.cpp")
    deps = [src, os.path.join(HERE, "..", "include", "color_balance_c.h"), os.path.join(HERE, "..", "include", "vp.h"), os.path.join(LIBDIR, "libvp.so")]
    if not force and not _stale(out, deps):
        return out
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", src, "-o", out, "-L" + LIBDIR, "-lvp", "-Wl,-rpath,$ORIGIN", "-lpthread"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_all(force=False, verbose=False):
    return [build_libvp(force, verbose), build_libcmf(force, verbose), build_libbalance(force, verbose)]


if __name__ == "__main__":
    if "--print-sources" in sys.argv:      # for the measurement builds under tools/: the one list of libvp's translation units
        print(" ".join(os.path.join(CSRC, s) for s in VP_SOURCES))
        sys.exit(0)
    print(build_all(force="--force" in sys.argv, verbose=True))
