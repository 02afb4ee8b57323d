"""Inputs and call helpers shared by tests/test_model_abi.py and tests/test_gpu_model.py: the sweep of point sets, the statement's
answer on each (computed once per process, tests/model_restate.py) and thin ctypes wrappers of the C entries of the motion models."""
import ctypes as C
import functools

import numpy as np

import model_restate as R

MODELS = (R.SIMILARITY, R.AFFINE, R.HOMOGRAPHY)
NAMES = {R.SIMILARITY: "similarity", R.AFFINE: "affine", R.HOMOGRAPHY: "homography"}


@functools.lru_cache(maxsize=None)
def library():
    from vision import _vp
    lib = C.CDLL(_vp.LIB_PATH)
    for name, (res, args) in _vp._SIGS.items():
        if name.startswith(("vp_model_", "vp_estimate_model_")) or name == "vp_last_error":
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


@functools.lru_cache(maxsize=None)
def pairs(n, model, outliers, seed=0):
    src, dst, good, H = R.make_pairs(n, model, outliers, seed)
    for a in (src, dst, good, H):
        a.flags.writeable = False
    return src, dst, good, H


def special(kind, model):
    """point sets on which there is no model, or on which many hypotheses are void"""
    r = np.random.default_rng(5)
    if kind == "collinear":                     # exactly on the line y = x / 2 + 3 in both sets (every coordinate a small integer or half)
        x = np.arange(40, dtype=np.float32) * 4
        src = np.stack([x, x / 2 + 3], 1)
        return src, src + np.float32(8)
    if kind == "identical":
        src = np.full((40, 2), 7.5, np.float32)
        return src, src.copy()
    src, dst, _, _ = (a.copy() for a in pairs(40, model, 0.3, 3))
    if kind == "duplicates":
        src[1::2] = src[0::2]
        dst[1::2] = dst[0::2]
    elif kind == "three_collinear":             # three quarters of the set on one line
        src[:30, 1] = src[:30, 0]
    elif kind == "flip":                        # half of the partners mirrored: many samples change orientation
        dst[::2, 0] = np.float32(2048) - dst[::2, 0]
    elif kind == "nan":
        src[7, 1] = np.nan
    elif kind == "exact":                       # n == m
        return src[:model + 2].copy(), dst[:model + 2].copy()
    else:
        raise KeyError(kind)
    return src, dst


def sweep():
    """(id, src, dst, model, keyword arguments) of every case both suites compare with the statement"""
    out = []
    for model in MODELS:
        m = model + 2
        for n in (m, m + 1, 63, 64, 65, 257):
            for share in (0.0, 0.3, 0.6):
                src, dst, _, _ = pairs(n, model, share)
                out.append((f"{NAMES[model]}-n{n}-out{int(share * 100)}", src, dst, model, {}))
        for kind in ("collinear", "identical"):
            src, dst = special(kind, model)
            out.append((f"{NAMES[model]}-{kind}", src, dst, model, {"max_iters": 300}))
        src, dst, _, _ = pairs(257, model, 0.0)
        out.append((f"{NAMES[model]}-first-round", src, dst, model, {"max_iters": 2000}))
        # so few inliers that 0.999999 asks for more than 600 hypotheses: inlier share ^ m below 0.0266
        src, dst, _, _ = pairs(65, model, (0.86, 0.75, 0.65)[model], 1)
        out.append((f"{NAMES[model]}-to-max-iters", src, dst, model, {"max_iters": 600, "confidence": 0.999999}))
        src, dst, _, _ = pairs(129, model, (0.86, 0.75, 0.65)[model], 2)
        out.append((f"{NAMES[model]}-later-round", src, dst, model, {"confidence": 0.999999}))
    return out


SWEEP = sweep()
SWEEP_IDS = [c[0] for c in SWEEP]


@functools.lru_cache(maxsize=None)
def _stated(key, model, threshold, max_iters, confidence, seed):
    src, dst = _ARRAYS[key]
    H, mask, count, taken, best_j = R.estimate(src, dst, model, threshold, max_iters, confidence, seed)
    mask.flags.writeable = False
    return H, mask, count, taken, best_j


_ARRAYS = {}


def stated(src, dst, model, threshold=3.0, max_iters=2000, confidence=0.99, seed=0):
    """the statement's answer, computed once per distinct input"""
    key = (src.tobytes(), dst.tobytes())
    _ARRAYS.setdefault(key, (src, dst))
    return _stated(key, model, float(threshold), int(max_iters), float(confidence), int(seed))


def call(entry, ctx, src, dst, model, threshold=3.0, max_iters=2000, confidence=0.99, seed=0, want_mask=True, n=None):
    """(return code, model bits uint64 (9,), mask uint8 (n,) or None, inlier count, hypotheses taken) of one of the three estimate
    entries; ctx is a context handle, or None for vp_estimate_model_host; src / dst are numpy arrays or device addresses"""
    lib = library()
    n = len(src) if n is None else n
    H = np.full(9, 7.25, np.float64)
    mask = np.full(n, 9, np.uint8) if want_mask else None
    ni, nh = C.c_int(-5), C.c_int(-5)
    p = lambda a: a.ctypes.data if isinstance(a, np.ndarray) else a
    args = (p(src), p(dst), n, model, threshold, max_iters, confidence, seed, H.ctypes.data, None if mask is None else mask.ctypes.data,
            C.addressof(ni), C.addressof(nh))
    rc = getattr(lib, entry)(*args) if ctx is None else getattr(lib, entry)(ctx, *args)
    return rc, H.view(np.uint64), mask, ni.value, nh.value


def same(got, want, what=""):
    """got: what `call` returned; want: what `stated` returned"""
    rc, hb, mask, count, taken = got
    H, wmask, wcount, wtaken, _ = want
    assert rc == 0, (what, rc, library().vp_last_error(None))
    assert (hb == R.bits(H)).all(), (what, "model", hb.view(np.float64).tolist(), H)
    assert mask is None or mask.tobytes() == wmask.tobytes(), (what, "mask", int(mask.sum()), int(wmask.sum()))
    assert (count, taken) == (wcount, wtaken), (what, "inliers, hypotheses", (count, taken), (wcount, wtaken))
