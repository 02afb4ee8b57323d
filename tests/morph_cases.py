"""Cases of the bit-plane morphology dispatch shared by tests/test_gpu_morph_dispatch.py, its child process
(tests/_morph_fallback_worker.py), tests/test_gpu_fuzz.py and tests/test_morph_plan_host.py: the switch widths read from the plan
table (tests/golden/morph_plan.txt, which tests/native/morph_plan_main.cpp prints from csrc/vp_morph_plan.h), the masks per shape,
and the comparisons with the oracle.  Nothing here needs a GPU until a check is called."""
import functools
import os

import numpy as np

import frames as F

HEIGHTS = (33, 65, 70, 129)          # 33: the last 32-row strip has one row; 65: the last 64-row strip has one row
# exactly one lap of 32 words; one valid bit in the second lap's word; one whole word in it; 4K; 128 words
COMMON_WIDTHS = (2048, 2049, 2112, 3840, 8192)
SEAM_COLS = (0, 63, 64, 2047, 2048, -1)
SEAM_ROWS = (0, 31, 32, 63, 64, -1)
ERODE, DILATE, OPEN, CLOSE = 0, 1, 2, 3      # libvp's and the oracle's codes alike


@functools.lru_cache(maxsize=None)
def _table():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "morph_plan.txt")
    plans, cases = {}, {}
    for line in open(path):
        f = line.split()
        if not f or f[0] == "#":
            continue
        kv = dict(x.split("=", 1) for x in f[1:] if "=" in x)
        if f[0].startswith("plan="):
            name = f[0][5:]
            plans[name] = {k: (None if v == "-" else 1 << 30 if v.startswith(">") else int(v)) for k, v in kv.items()}
        elif f[0] == "case":
            key = (kv.pop("plan"), int(kv.pop("h")), int(kv.pop("w")))
            if "refused" in f:
                cases[key] = "refused"
            else:
                kv["launches"] = int(kv["launches"])
                cases[key] = kv
    return plans, cases


def plan_table():
    """name -> {stages, halo (sum of the vertical extents), shape, strip64_last, sym_last, one_launch_last, accepted_last}"""
    return _table()[0]


def plan_case(name, h, w):
    return _table()[1][(name, h, w)]


def switch_widths(name):
    """The last width on each side of every switch of the named plan (below 8320): 64- to 32-row strips, specialised to runtime-plan
    kernel, one launch to two, accepted to refused."""
    out = []
    for key in ("strip64_last", "sym_last", "one_launch_last", "accepted_last"):
        v = plan_table()[name][key]
        if v is not None and v + 1 <= 8320:
            out += [v, v + 1]
    return sorted(set(out))


def widths_for(name):
    return sorted(set(COMMON_WIDTHS) | set(switch_widths(name)))


def all_switch_widths():
    """every switch width of the 12 specialised shapes"""
    names = [n for n, p in plan_table().items() if p["shape"] is not None and not n.startswith("chain")]
    return sorted({w for n in names for w in switch_widths(n)})


def seam_mask(h, w):
    """Set pixels on an empty image at SEAM_COLS x SEAM_ROWS (the positions that fit the shape): the first and last column of a
    word, of a lap of 32 words and of the image, the first and last row of a 32- and a 64-row strip and of the image.  A shift
    across a word, lap or strip seam shows on the far side; 255 - seam_mask has holes at the same places."""
    m = np.zeros((h, w), np.uint8)
    cols = sorted({c % w for c in SEAM_COLS if -1 <= c < w})
    rows = sorted({r % h for r in SEAM_ROWS if -1 <= r < h})
    m[np.ix_(rows, cols)] = 255
    return m


@functools.lru_cache(maxsize=8)
def masks(h, w):
    """[(name, mask)]: random masks at densities 0.1, 0.5 and 0.9 and the constructed one with its complement.  Made once per shape
    and shared: nothing may write to them."""
    rng = np.random.default_rng(h * 100003 + w)
    out = [("p%.1f" % p, F.random_mask(rng, h, w, p)) for p in (0.1, 0.5, 0.9)]
    s = seam_mask(h, w)
    out += [("seam-pixels", s), ("seam-holes", 255 - s)]
    for _, m in out:
        m.setflags(write=False)
    return out


# name of the plan in the table -> (operation, kernel side)
SINGLE_OPS = {"erode3": (ERODE, 3), "dilate3": (DILATE, 3), "open3": (OPEN, 3), "close3": (CLOSE, 3),
              "erode5": (ERODE, 5), "dilate5": (DILATE, 5), "open5": (OPEN, 5), "close5": (CLOSE, 5)}
CHAIN_PAIRS = {"open3+close3": [(OPEN, 3, 3, 1), (CLOSE, 3, 3, 1)], "close3+open3": [(CLOSE, 3, 3, 1), (OPEN, 3, 3, 1)],
               "open5+close5": [(OPEN, 5, 5, 1), (CLOSE, 5, 5, 1)], "close5+open5": [(CLOSE, 5, 5, 1), (OPEN, 5, 5, 1)]}
# plans no specialised kernel takes: (table name for the widths, operation, kernel (kw, kh), iterations)
GENERAL_OPS = [("open7x7", OPEN, (7, 7), 1), ("close4x2", CLOSE, (4, 2), 1), ("erode9x3", ERODE, (9, 3), 1), ("erode3x3i3", ERODE, (3, 3), 3)]


def transform_op(op):
    from vision.utils import transform as T
    return {ERODE: T.erode, DILATE: T.dilate, OPEN: T.morph_remove_noise, CLOSE: T.morph_close_holes}[op]


def check_single(oracle, m, op, kw, kh, iterations=1, device=True, what=""):
    """One operation on a host mask and, with `device`, on a device-resident mask known to be 0/255 (binary_hint = 1: no flag comes
    back), both against the oracle."""
    from vision import _vp
    from vision.devmat import DeviceMat
    k = np.ones((kh, kw), np.uint8)
    ref = oracle.morph(op, m, k, iterations=iterations, fast=True)
    got = transform_op(op)(m, k, iterations=iterations)
    assert np.array_equal(np.asarray(got), ref), (what, m.shape, op, kw, kh, iterations, "host mask", _first_diff(np.asarray(got), ref))
    if device:
        dm = DeviceMat.from_host(_vp.default_context(), m, binary=True)
        out = transform_op(op)(dm, k, iterations=iterations)
        assert isinstance(out, DeviceMat) and out.binary
        got = out.host_copy()
        assert np.array_equal(got, ref), (what, m.shape, op, kw, kh, iterations, "device mask", _first_diff(got, ref))


def _first_diff(a, b):
    if a.shape != b.shape:
        return ("shape", a.shape, b.shape)
    d = np.argwhere(a != b)
    return (len(d), tuple(int(v) for v in d[0])) if len(d) else None


def frames_of(masks_):
    """BGR frames whose grey level is the mask: all three channels equal"""
    return np.ascontiguousarray(np.repeat(np.stack(masks_)[..., None], 3, axis=3))


def check_chain(oracle, masks_, morph, ccl, source, what="", max_labels=8192):
    """The chain on frames made from the masks (BGR2GRAY, bounds 128..255) against the oracle run step by step: the threshold mask
    is the mask, then cleaned, nlabels / labels / stats / centroids of the labelled mask (ccl = 1: cleaned, 2: threshed) and the
    contours of `source`."""
    from vision import _vp
    from vision.utils import chain
    fr = frames_of(masks_)
    out = chain.run_chain(fr, _vp.BGR2GRAY, (128, 0, 0), (255, 255, 255), morph, ccl=ccl, max_labels=max_labels,
                          contours=dict(source=source, mode=1, method=2, max_contours=4096, max_points=1 << 16))
    for f, m in enumerate(masks_):
        tag = (what, m.shape, f, morph, ccl, source)
        assert np.array_equal(out["threshed"][f], m), tag + ("threshed", _first_diff(out["threshed"][f], m))
        cl = m
        for op, kw, kh, it in morph:
            cl = oracle.morph(op, cl, np.ones((kh, kw), np.uint8), iterations=it, fast=True)
        assert np.array_equal(out["cleaned"][f], cl), tag + ("cleaned", _first_diff(out["cleaned"][f], cl))
        on, olab, ost, oce = oracle.ccl(cl if ccl == 1 else m, block=_vp.CCL_BLOCK2X2)
        assert int(out["nlabels"][f]) == on, tag + ("nlabels", int(out["nlabels"][f]), on)
        assert np.array_equal(out["labels"][f], olab), tag + ("labels",)
        k = min(on, max_labels)
        assert np.array_equal(out["stats"][f][:k], ost[:k]), tag + ("stats",)
        assert np.array_equal(out["centroids"][f][:k].view(np.uint64), oce[:k].view(np.uint64)), tag + ("centroids",)
        exp, eh = oracle.find_contours(cl if source == "cleaned" else m, 1, 2, with_holes=True)
        got, gh = out["contours"][f]
        assert len(got) == len(exp) and all(np.array_equal(a, b) for a, b in zip(got, exp)) and np.array_equal(gh, eh), tag + ("contours", len(got), len(exp))


def chain_batch(h, w, first=0):
    """three different masks of one shape (a batch whose last strip is partial when h is no multiple of the strip height)"""
    ms = [m for _, m in masks(h, w)]
    return [ms[(first + i) % len(ms)] for i in range(3)]


def fallback_cases(oracle):
    """What the child process runs with VP_NO_SYM=1 or VP_MORPH_STRIP32=1 (read once per process, so no in-process test reaches
    them): the single operations and the chains of two on three common shapes.  Yields descriptions as it goes."""
    for h, w in ((65, 257), (129, 2112), (70, 3840)):
        for name, (op, k) in SINGLE_OPS.items():
            for mname, m in masks(h, w):
                check_single(oracle, m, op, k, k, what=(name, mname))
            yield "%s %dx%d" % (name, h, w)
        for name, morph in CHAIN_PAIRS.items():
            check_chain(oracle, chain_batch(h, w, 1), morph, 1, "cleaned", what=name)
            yield "%s %dx%d" % (name, h, w)
