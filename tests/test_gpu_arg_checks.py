"""The argument checks that a host / device (/ batch) pair of entry points shares: every bad call gets the same code from every
form of its pair.  One row per failing condition, made straight through the C ABI on 8x8 images; the rows that only one form has
(stride below a row, destination over the source, frame count, max_keep == 0) name that form.  A rejected call launches nothing;
each family also makes one good 8x8 call per form.  The expected codes are those of include/vp.h: VP_ERR_INVALID for an argument
that is wrong in itself, VP_ERR_UNSUPPORTED for a valid request outside what the kernels cover, and where one call breaks two
rules, the rule tested first decides."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED = 0, -1, -4
NAN, INF = float("nan"), float("inf")
SRC, DST = "src", "dst"      # stand for the form's own 8x8 buffers: host arrays for the host form, device memory for the others


class _Buffers:
    def __init__(self, vp):
        self.vp, self.L, self.ctx = vp, vp.lib(), vp.default_context().handle
        rng = np.random.default_rng(5)
        self.h_src = rng.integers(0, 256, 1024, dtype=np.uint8)
        self.h_dst = np.zeros(1024, np.uint8)
        self.h_word = np.zeros(8, np.uint8)                      # a double / an int the host forms hand back
        self.h_keep = np.zeros(16, np.int32)
        self.h_boxes = np.array([[0, 0, 4, 4], [1, 1, 5, 5], [20, 20, 24, 24], [40, 40, 41, 41]], np.float32)
        self.h_scores = np.array([0.9, 0.8, 0.7, 0.6], np.float32)
        self.m23 = np.array([1, 0, 0, 0, 1, 0], np.float64)
        self.cval = np.zeros(4, np.uint8)
        self.dev = []
        self.d_src, self.d_dst, self.d_word, self.d_keep = (self._alloc(n) for n in (1024, 1024, 64, 64))
        self.d_boxes, self.d_scores = self._alloc(64), self._alloc(16)
        for d, h in ((self.d_src, self.h_src), (self.d_boxes, self.h_boxes), (self.d_scores, self.h_scores)):
            assert self.L.vp_memcpy_h2d(self.ctx, d, vp.ptr(h), h.nbytes) == OK

    def _alloc(self, n):
        p = C.c_void_p()
        assert self.L.vp_dev_alloc(self.ctx, n, C.byref(p)) == OK
        self.dev.append(p.value)
        return p.value

    def close(self):
        assert self.L.vp_synchronize(self.ctx) == OK
        for p in self.dev:
            self.L.vp_dev_free(self.ctx, p)

    def image(self, form, which):
        """SRC / DST -> the form's buffer; "src" as a destination -> the source itself (overlap); anything else as given."""
        host = form == "host"
        if which == SRC:
            return (self.vp.ptr(self.h_src) if host else self.d_src)
        if which == DST:
            return (self.vp.ptr(self.h_dst) if host else self.d_dst)
        return which


@pytest.fixture(scope="module")
def B(vp):
    b = _Buffers(vp)
    yield b
    b.close()


# ---- one caller per family: a = the good arguments with the row's changes applied ---------------------------------------------------

def _threshold(B, form, a):
    f = B.L.vp_threshold_u8 if form == "host" else B.L.vp_threshold_u8_dev
    return f(B.ctx, B.image(form, a["src"]), a["n"], a["thresh"], a["maxval"], a["type"], B.image(form, a["dst"]))


def _otsu(B, form, a):
    if form == "host":
        return B.L.vp_otsu_threshold_u8(B.ctx, B.image(form, a["src"]), a["n"], a["maxval"], a["type"], B.vp.ptr(B.h_word), B.image(form, a["dst"]))
    return B.L.vp_otsu_threshold_dev(B.ctx, B.image(form, a["src"]), a["n"], a["maxval"], a["type"], B.d_word, B.image(form, a["dst"]))


def _blur(B, form, a):
    s, d = B.image(form, a["src"]), B.image(form, a["dst"])
    if form == "host":
        return B.L.vp_gaussian_blur_u8(B.ctx, s, a["w"], a["h"], a["cn"], a["kw"], a["kh"], a["s1"], a["s2"], d)
    return B.L.vp_gaussian_blur_dev(B.ctx, s, a["stride"], a["w"], a["h"], a["cn"], a["kw"], a["kh"], a["s1"], a["s2"], d)


def _resize(B, form, a):
    s, d = B.image(form, a["src"]), B.image(form, a["dst"])
    if form == "host":
        return B.L.vp_resize_u8_scaled(B.ctx, s, a["w"], a["h"], a["cn"], a["dw"], a["dh"], a["isx"], a["isy"], d)
    return B.L.vp_resize_dev(B.ctx, s, a["stride"], a["w"], a["h"], a["cn"], a["dw"], a["dh"], a["isx"], a["isy"], d)


def _warp(B, form, a):
    s, d = B.image(form, a["src"]), B.image(form, a["dst"])
    m = None if a["m23"] is None else np.array(a["m23"], np.float64)
    tail = (B.vp.ptr(m), a["flags"], a["border"], B.vp.ptr(B.cval), d, a["dw"], a["dh"])
    if form == "host":
        return B.L.vp_warp_affine_u8(B.ctx, s, a["w"], a["h"], a["cn"], *tail)
    return B.L.vp_warp_affine_dev(B.ctx, s, a["stride"], a["w"], a["h"], a["cn"], *tail)


def _adaptive(kind):
    def call(B, form, a):
        s, d = B.image(form, a["src"]), B.image(form, a["dst"])
        tail = (a["w"], a["h"], a["max_value"], a["type"], a["block"], a["c"], d)
        if form == "host":
            return getattr(B.L, f"vp_adaptive_threshold_{kind}_u8")(B.ctx, s, *tail)
        if form == "dev":
            return getattr(B.L, f"vp_adaptive_threshold_{kind}_dev")(B.ctx, s, a["stride"], *tail)
        return B.L.vp_adaptive_threshold_gaussian_batch_dev(B.ctx, s, a["stride"], a["fstride"], a["n"], *tail)
    return call


def _canny(B, form, a):
    s, d = B.image(form, a["src"]), B.image(form, a["dst"])
    if form == "host":
        return B.L.vp_canny_u8(B.ctx, s, a["w"], a["h"], a["cn"], a["t1"], a["t2"], d)
    return B.L.vp_canny_u8_dev(B.ctx, s, a["stride"], a["w"], a["h"], a["cn"], a["t1"], a["t2"], d)


def _nms(B, form, a):
    host = form == "host"
    pick = lambda v, h, d: (B.vp.ptr(h) if host else d) if v == "own" else v   # noqa: E731
    f = B.L.vp_nms_f32 if host else B.L.vp_nms_dev
    return f(B.ctx, pick(a["boxes"], B.h_boxes, B.d_boxes), pick(a["scores"], B.h_scores, B.d_scores), a["n"], 0.5, 0, a["max_keep"],
             pick(a["keep"], B.h_keep, B.d_keep), pick(a["n_keep"], B.h_word, B.d_word))


_IMG3 = dict(src=SRC, dst=DST, w=8, h=8, cn=3, stride=24)
_IMG1 = dict(src=SRC, dst=DST, w=8, h=8, stride=8)
_ADAPT = dict(_IMG1, max_value=255.0, type=0, block=3, c=2.0, fstride=64, n=1)
FAMILIES = {
    "threshold": (_threshold, ("host", "dev"), dict(src=SRC, dst=DST, n=64, thresh=100.0, maxval=255.0, type=0)),
    "otsu": (_otsu, ("host", "dev"), dict(src=SRC, dst=DST, n=64, maxval=255.0, type=0)),
    "blur": (_blur, ("host", "dev"), dict(_IMG3, kw=3, kh=5, s1=0.0, s2=0.0)),
    "resize": (_resize, ("host", "dev"), dict(_IMG3, dw=4, dh=4, isx=0.5, isy=0.5)),
    "warp": (_warp, ("host", "dev"), dict(_IMG3, m23=(1, 0, 0, 0, 1, 0), flags=0, border=0, dw=8, dh=8)),
    "adaptive_mean": (_adaptive("mean"), ("host", "dev"), _ADAPT),
    "adaptive_gaussian": (_adaptive("gaussian"), ("host", "dev", "batch"), _ADAPT),
    "canny": (_canny, ("host", "dev"), dict(_IMG3, t1=50.0, t2=100.0)),
    "nms": (_nms, ("host", "dev"), dict(boxes="own", scores="own", n=4, max_keep=4, keep="own", n_keep="own")),
}

_NULLS = [(dict(src=None), INVALID), (dict(dst=None), INVALID)]
_SIZE = [(dict(w=0), INVALID), (dict(h=0), INVALID), (dict(h=65536), INVALID)]
_CN = [(dict(cn=0), INVALID), (dict(cn=5), INVALID)]
_TYPE5 = [(dict(type=5), INVALID), (dict(type=-1), INVALID)]
_STRIDE3 = [(dict(stride=23), INVALID, ("dev",)), (dict(dst=SRC), INVALID, ("dev",))]
_ADAPT_ROWS = _NULLS + _SIZE + [
    (dict(type=2), INVALID), (dict(max_value=NAN), INVALID), (dict(max_value=INF), INVALID), (dict(c=NAN), INVALID), (dict(c=2e6), INVALID),
    (dict(block=4), INVALID), (dict(block=1), INVALID),
    (dict(type=2, block=4), INVALID),
    (dict(max_value=-1.0), OK),                                   # cv2 gives zeros: a memset in every form
]
# (changes to the good call, expected code[, the forms the row is for: all of the pair's when absent])
ROWS = {
    "threshold": _NULLS + _TYPE5 + [(dict(n=0), INVALID), (dict(thresh=NAN), INVALID), (dict(maxval=NAN), INVALID),
                                    (dict(dst=SRC), INVALID, ("dev",))],
    "otsu": _NULLS + _TYPE5 + [(dict(n=0), INVALID), (dict(n=1 << 32), INVALID), (dict(maxval=NAN), INVALID), (dict(dst=SRC), INVALID, ("dev",))],
    "blur": _NULLS + _SIZE + _CN + _STRIDE3 + [(dict(kw=0), INVALID), (dict(kh=0), INVALID), (dict(kw=4), INVALID), (dict(kh=2), INVALID),
                                                (dict(kw=513), INVALID), (dict(kh=513), INVALID)],
    "resize": _NULLS + _CN + _STRIDE3 + [
        (dict(w=0), INVALID), (dict(h=0), INVALID), (dict(dw=0), INVALID), (dict(dh=0), INVALID), (dict(dh=65536), INVALID),
        (dict(isx=NAN), INVALID), (dict(isy=INF), INVALID), (dict(isx=0.0), INVALID), (dict(isy=-1.0), INVALID),
        (dict(isx=0.0, isy=0.0), INVALID, ("host",)), (dict(isx=0.0, isy=0.0), OK, ("dev",)),      # the device form derives the scale from the sizes
    ],
    "warp": _NULLS + _CN + _STRIDE3 + [
        (dict(m23=None), INVALID), (dict(w=0), INVALID), (dict(h=0), INVALID), (dict(dw=0), INVALID), (dict(dh=0), INVALID), (dict(dh=65536), INVALID),
        (dict(flags=1), INVALID), (dict(border=2), INVALID), (dict(m23=(1, 0, NAN, 0, 1, 0)), INVALID), (dict(m23=(1, 0, 0, 0, INF, 0)), INVALID),
    ],
    "adaptive_mean": _ADAPT_ROWS + [
        (dict(block=153), UNSUPPORTED), (dict(type=2, block=153), INVALID),
        (dict(stride=7), INVALID, ("dev",)), (dict(dst=SRC), INVALID, ("dev",)),
        (dict(block=153, stride=7), UNSUPPORTED, ("dev",)),       # the block size is tested before the stride
    ],
    "adaptive_gaussian": _ADAPT_ROWS + [
        (dict(block=513), UNSUPPORTED), (dict(type=2, block=513), INVALID),
        (dict(stride=7), INVALID, ("dev", "batch")), (dict(block=513, stride=7), UNSUPPORTED, ("dev", "batch")),
        (dict(n=0), INVALID, ("batch",)), (dict(n=65536), INVALID, ("batch",)), (dict(n=2, fstride=63), INVALID, ("batch",)),
    ],
    "canny": _NULLS + _SIZE + _CN + [(dict(t1=NAN), INVALID), (dict(t2=INF), INVALID), (dict(w=32768, h=32769), INVALID),
                                      (dict(stride=23), INVALID, ("dev",))],
    "nms": [(dict(n=-1), INVALID), (dict(max_keep=-1), INVALID), (dict(n_keep=None), INVALID), (dict(boxes=None), INVALID), (dict(scores=None), INVALID),
            (dict(keep=None), INVALID),
            (dict(max_keep=0), OK, ("host",)), (dict(max_keep=0), INVALID, ("dev",))],     # the host form answers "nothing kept"
}


def _row_id(family, row):
    what = ",".join(f"{k}={v}" for k, v in row[0].items())
    return f"{family}[{what}]" + ("@" + "+".join(row[2]) if len(row) > 2 else "")


_CASES = [(fam, row) for fam in FAMILIES for row in ROWS[fam]]


@pytest.mark.parametrize("family,row", _CASES, ids=[_row_id(f, r) for f, r in _CASES])
def test_bad_call_same_code_from_every_form(B, family, row):
    call, forms, good = FAMILIES[family]
    want = row[1]
    got = {form: call(B, form, dict(good, **row[0])) for form in (row[2] if len(row) > 2 else forms)}
    print(family, row[0], got)
    assert got == {form: want for form in got}
    if want != OK:
        assert B.L.vp_last_error(B.ctx)           # a rejected call leaves a message


@pytest.mark.parametrize("family", list(FAMILIES))
def test_good_call_every_form(B, family):
    call, forms, good = FAMILIES[family]
    for form in forms:
        assert call(B, form, dict(good)) == OK, form
    assert B.L.vp_synchronize(B.ctx) == OK
