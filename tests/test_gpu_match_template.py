"""GPU suite for cv2.matchTemplate (vp_match_template_*, vision.utils.feature.match_template / best_match, vision.cv2_facade).

Every comparison is exact: tobytes() equality against tests/match_template_restate.py, never against the library under test; the sums
of the statement are cached per input.  Each map is taken three ways - the host entry, the device entry with padded strides on the
image, the template and the result (rows off word boundaries), the facade on a device image - and the three must agree with the
statement.  The shapes are the smallest at which a kernel can go wrong: every tail of a dot word, the tile's edges, the chunk's edges
and the switch between one piece and chunks, all read from csrc/vp_match_plan.h, and the size bound where a signed sum overflows."""
import functools
import os
import re

import numpy as np
import pytest

import match_template_restate as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PLAN = open(os.path.join(ROOT, "cuauv-vision-pipeline_amd", "csrc", "vp_match_plan.h")).read()
_num = lambda n: int(re.search(r"#define " + n + r" (\d+)", _PLAN).group(1))
TILE_W, TILE_H, CHUNK_ROWS, CHUNK_WORDS = _num("MT_TILE_W"), _num("MT_TILE_H"), _num("MT_CHUNK_ROWS"), _num("MT_CHUNK_WORDS")
assert "P->one_piece = P->row_chunks == 1 && P->col_chunks == 1;" in _PLAN and "(th + MT_CHUNK_ROWS - 1) / MT_CHUNK_ROWS" in _PLAN

_INPUTS = {}


def _key(img, templ):
    k = (img.shape, templ.shape, img.tobytes(), templ.tobytes())
    _INPUTS.setdefault(k, (img, templ))
    return k


@functools.lru_cache(maxsize=None)
def _sums(key):
    return R.sums(*_INPUTS[key])


def _expect(img, templ, method):
    return R.finish(*_sums(_key(img, templ)), method)


def _random(h, w, cn, seed=0):
    a = np.random.default_rng(h * 8191 + w * 131 + cn * 7 + seed).integers(0, 256, (h, w, cn), dtype=np.uint8)
    return a if cn > 1 else a[:, :, 0]


def _dev(ctx, arr):
    from vision.devmat import DeviceMat
    return DeviceMat.from_host(ctx, arr)


def _padded(ctx, arr, pad, fill):
    """the array in rows of pad more bytes on the device, and its stride in bytes"""
    rows = arr.reshape(arr.shape[0], -1)
    wide = np.full((rows.shape[0], rows.shape[1] + pad), fill, np.uint8)
    wide[:, :rows.shape[1]] = rows
    return _dev(ctx, wide), wide.shape[1]


def _device_entry(vp, img, templ, method, spad=5, tpad=3, dpad=3):
    """vp_match_template_dev on padded rows; the result's columns, after a check that its padding kept its fill"""
    ctx = vp.default_context()
    (h, w), (th, tw), cn = img.shape[:2], templ.shape[:2], 1 if img.ndim == 2 else img.shape[2]
    rh, rw = h - th + 1, w - tw + 1
    src, stride = _padded(ctx, img, spad, 255)          # 255s in the padding: they would count, if they were read
    tpl, tstride = _padded(ctx, templ, tpad, 255)
    dst = _dev(ctx, np.full((rh, rw + dpad), 90, np.float32))
    rc = vp.lib().vp_match_template_dev(ctx.handle, src.dev_ptr, stride, w, h, cn, tpl.dev_ptr, tstride, tw, th, method, dst.dev_ptr, (rw + dpad) * 4)
    vp.check(rc, ctx.handle)
    got = dst.host_copy()
    assert (got[:, rw:] == 90).all(), "the result's padding was written"
    return np.ascontiguousarray(got[:, :rw])


def _three_ways(vp, img, templ, methods=R.METHODS):
    from vision import cv2_facade as f
    from vision.devmat import DeviceMat
    from vision.utils import feature
    ctx = vp.default_context()
    src = _dev(ctx, img)
    for method in methods:
        exp = _expect(img, templ, method)
        tag = (img.shape, templ.shape, method)
        got = feature.match_template(img, templ, method)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == exp.shape and got.tobytes() == exp.tobytes(), tag + ("host",)
        assert _device_entry(vp, img, templ, method).tobytes() == exp.tobytes(), tag + ("device, padded strides",)
        dgot = f.matchTemplate(src, templ, method)
        assert isinstance(dgot, DeviceMat) and dgot.dtype == np.float32 and dgot.shape == exp.shape
        assert dgot.host(writable=False).tobytes() == exp.tobytes(), tag + ("facade, device image",)
    assert src._host is None, "a host copy of the source was made"


@pytest.mark.parametrize("cn", (1, 3, 4))
def test_every_method_and_every_tail_of_a_dot_word(vp, cn):
    img = _random(11, 23, cn)
    for tw in (1, 2, 3, 4, 5, 7, 8, 9):
        for th in (1, 2, 5):
            y, x = (3, 6) if tw < 9 else (2, 5)
            _three_ways(vp, img, img[y:y + th, x:x + tw].copy())


def test_two_channels(vp):
    img = _random(9, 14, 2)
    _three_ways(vp, img, img[2:5, 3:8].copy())


@pytest.mark.parametrize("cn", (1, 3))
def test_image_sizes_round_the_tile(vp, cn):
    tw, th = 3, 2
    for dw in (-1, 0, 1):
        for dh in (-1, 0, 1):
            img = _random(TILE_H + th - 1 + dh, TILE_W + tw - 1 + dw, cn)
            _three_ways(vp, img, img[5:5 + th, 70:70 + tw].copy(), (R.SQDIFF, R.CCORR_NORMED, R.CCOEFF_NORMED))
    img = _random(2 * TILE_H + th, 2 * TILE_W + tw, cn)              # 2 x 2 tiles and one more result either way: 3 x 3 blocks
    _three_ways(vp, img, img[40:40 + th, 200:200 + tw].copy(), (R.CCORR, R.CCOEFF_NORMED))


def test_narrow_results(vp):
    for cn in (1, 3, 4):
        img = _random(6, 7, cn)
        _three_ways(vp, img, img.copy())                                 # 1 x 1: the template is the image
        for rw in (1, 2, 3):
            _three_ways(vp, img, img[1:4, 0:7 - rw + 1].copy())
            _three_ways(vp, img, img[0:6 - rw + 1, 2:5].copy())         # the same for result heights


def test_template_rows_round_the_chunk_and_the_switch_to_chunks(vp):
    """th = MT_CHUNK_ROWS is the last template in one piece, th + 1 the first in chunks; 2 chunks + 1 row has a last chunk of one row"""
    for cn in (1, 3):
        for th in (CHUNK_ROWS - 1, CHUNK_ROWS, CHUNK_ROWS + 1, 2 * CHUNK_ROWS, 2 * CHUNK_ROWS + 1):
            img = _random(th + 3, 12, cn, seed=th)
            _three_ways(vp, img, img[1:1 + th, 2:9].copy(), (R.CCORR, R.SQDIFF_NORMED, R.CCOEFF_NORMED))


def test_template_words_round_the_chunk_and_the_switch_to_chunks(vp):
    """a template row of 4 * MT_CHUNK_WORDS bytes is the last in one piece; one byte more starts a second chunk of words"""
    row = 4 * CHUNK_WORDS
    for cn, tws in ((1, (row - 1, row, row + 1, 2 * row + 1)), (3, (row // 3, row // 3 + 1)), (4, (row // 4, row // 4 + 1))):
        for tw in tws:
            img = _random(4, tw + 3, cn, seed=tw)
            _three_ways(vp, img, img[1:3, 2:2 + tw].copy(), (R.CCORR, R.CCOEFF_NORMED))
    img = _random(CHUNK_ROWS + 4, row + 5, 1)                            # chunks both ways: 2 x 2 of them
    _three_ways(vp, img, img[1:2 + CHUNK_ROWS, 2:3 + row].copy(), (R.CCORR, R.SQDIFF))


@pytest.mark.parametrize("cn,side", ((1, 256), (4, 128)))
def test_the_size_bound_where_a_signed_sum_overflows(vp, cn, side):
    shape = (side, side + 1) if cn == 1 else (side, side + 1, cn)
    img = np.full(shape, 255, np.uint8)
    templ = np.full((side, side) if cn == 1 else (side, side, cn), 255, np.uint8)
    assert side * side * cn == R.MAX_ELEMS
    c = _expect(img, templ, R.CCORR)
    assert c.shape == (1, 2) and (c == np.float32(4261478400)).all() and 4261478400 > 2 ** 31
    assert (_expect(img, templ, R.SQDIFF) == 0).all() and (_expect(img, templ, R.CCOEFF_NORMED) == 1).all()
    _three_ways(vp, img, templ, (R.CCORR, R.SQDIFF, R.CCOEFF_NORMED))
    img = img.copy()
    img[side // 2, 0] = 254                                          # not a constant window any more: the sums just below the bound
    templ = templ.copy()
    templ[0, side - 1] = 0
    _three_ways(vp, img, templ, (R.CCORR, R.SQDIFF, R.CCOEFF_NORMED))


def test_the_branch_inputs_of_the_statement(vp):
    import test_match_template_statement as S
    img = S.branch_image()
    templ = img[3:7, 4:9].copy()
    met = set()
    for m in R.NORMED:
        met |= set(np.unique(R.branches(img, templ, m)).tolist())
    assert met == {0, 1, 2, 3}
    _three_ways(vp, img, templ, R.NORMED)
    _three_ways(vp, img, np.full((4, 5), 7, np.uint8), R.NORMED)
    far_img, far_templ = S.far_pair()
    assert (R.branches(far_img, far_templ, R.SQDIFF_NORMED) == 3).all()
    _three_ways(vp, far_img, far_templ, R.NORMED)


def test_best_match_without_a_host_visit(vp, monkeypatch):
    from vision.devmat import DeviceMat
    from vision.utils import feature
    ctx = vp.default_context()
    img = _random(40, 150, 3) >> 2                                       # a dim frame, so that plain CCORR peaks on the bright patch too
    img[17:26, 131:142] = 128 + (_random(9, 11, 3, seed=9) >> 1)
    templ = img[17:26, 131:142].copy()                                   # found in the second tile of results
    src = _dev(ctx, img)

    def no_host(self, *a, **k):
        raise AssertionError("an image visited the host")
    monkeypatch.setattr(DeviceMat, "host", no_host)
    monkeypatch.setattr(DeviceMat, "host_copy", no_host)
    for method in R.METHODS:
        got = feature.best_match(src, templ, method)
        assert got == R.best_match(img, templ, method), method
        assert got[0] == (131, 17) and type(got[1]) is float, method


def test_best_match_ties_go_to_the_first_pixel(vp):
    from vision.utils import feature
    ctx = vp.default_context()
    img = np.zeros((20, 140), np.uint8)
    patch = _random(3, 4, 1, seed=5) | 1
    for y, x in ((12, 130), (5, 9), (5, 100), (12, 3)):
        img[y:y + 3, x:x + 4] = patch
    for method in R.METHODS:
        exp = R.best_match(img, patch, method)
        assert exp[0] == (9, 5), method
        assert feature.best_match(_dev(ctx, img), patch, method) == exp == feature.best_match(img, patch, method), method
    flat = np.full((5, 6), 9, np.uint8)
    for method in R.METHODS:                                             # every score equal: the first pixel of the map
        assert feature.best_match(_dev(ctx, flat), flat[:2, :3].copy(), method)[0] == (0, 0)


def test_a_template_cropped_from_a_device_image(vp):
    from vision import cv2_facade as f
    from vision.devmat import DeviceMat
    from vision.utils import feature
    ctx = vp.default_context()
    for cn in (1, 3):
        prev, cur = _random(30, 41, cn, seed=1), _random(30, 41, cn, seed=2)
        cur[9:16, 20:29] = prev[4:11, 13:22]
        dprev, dcur = _dev(ctx, prev), _dev(ctx, cur)
        crop = feature.DeviceCrop(dprev, 13, 4, 9, 7)
        for method in R.METHODS:
            exp = _expect(cur, prev[4:11, 13:22].copy(), method)
            got = f.matchTemplate(dcur, crop, method)
            assert isinstance(got, DeviceMat) and got.host(writable=False).tobytes() == exp.tobytes(), (cn, method)
            assert feature.match_template(dcur, _dev(ctx, prev[4:11, 13:22].copy()), method).host(writable=False).tobytes() == exp.tobytes()
        assert feature.best_match(dcur, crop, f.TM_SQDIFF) == ((20, 9), 0.0)
        assert dprev._host is None, "the cropped image visited the host"
        exp = _expect(cur, prev[4:11, 13:22].copy(), f.TM_CCOEFF_NORMED)        # a host image reads the window from the host copy
        assert feature.match_template(cur, crop).tobytes() == exp.tobytes()


def test_facade_numpy_in_numpy_out_and_result(vp):
    from vision import cv2_facade as f
    img = _random(17, 33, 3)
    templ = img[4:9, 10:17].copy()
    exp = _expect(img, templ, f.TM_CCOEFF_NORMED)
    got = f.matchTemplate(img, templ, f.TM_CCOEFF_NORMED)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.tobytes() == exp.tobytes()
    res = np.zeros(exp.shape, np.float32)
    assert f.matchTemplate(img, templ, f.TM_CCOEFF_NORMED, res) is res and res.tobytes() == exp.tobytes()
    assert f.matchTemplate(img, templ, f.TM_SQDIFF, result=None, mask=None).tobytes() == _expect(img, templ, f.TM_SQDIFF).tobytes()
    view = np.zeros((17, 40, 3), np.uint8)[:, 2:35]
    view[:] = img
    assert f.matchTemplate(view, img[4:9, 10:17], f.TM_CCORR).tobytes() == _expect(img, templ, f.TM_CCORR).tobytes()
    assert f.minMaxLoc(got)[3] == (10, 4)
