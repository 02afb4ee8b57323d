"""Seeded int16 images for the speckle-filter tests and the one list of cases the GPU test walks and tests/test_speckle_cases.py checks.
The sizes and positions that straddle a tile come from vp_filter_speckles_plan, not from constants here."""
import numpy as np

import speckle_restate as R

FAR = 1000          # a value no max_diff used here links with the small ones


def lib_plan(w, h):
    """vp_filter_speckles_plan as a dict (host only: no device, no context)"""
    import ctypes as C
    from vision import _vp
    geom, ws = (C.c_int32 * 5)(), C.c_size_t()
    _vp.check(_vp.lib().vp_filter_speckles_plan(w, h, C.byref(ws), geom))
    return dict(ws_bytes=ws.value, tile_w=geom[0], tile_h=geom[1], grid=(geom[2], geom[3]), lds_bytes=geom[4])


def tile():
    p = lib_plan(64, 64)
    assert p["tile_w"] == p["tile_h"]
    return p["tile_w"]


def noise(h, w, levels, seed, holes=0.0, new_val=-16):
    rng = np.random.default_rng(seed)
    img = np.asarray(levels, np.int16)[rng.integers(0, len(levels), (h, w))]
    if holes:
        img[rng.random((h, w)) < holes] = new_val
    return img


def serpentine(h, w, value=100, other=FAR):
    """a one-pixel path over every even row, joined at alternating ends on the odd rows; h odd.  Returns the image and the path's length"""
    assert h % 2 == 1
    img = np.full((h, w), other, np.int16)
    img[0::2, :] = value
    for k, y in enumerate(range(1, h, 2)):
        img[y, w - 1 if k % 2 == 0 else 0] = value
    return img, (h + 1) // 2 * w + h // 2


def ring(T):
    """a closed 4 x 4 ring of 12 pixels around the corner where four tiles meet, on a far background"""
    img = np.full((2 * T, 2 * T), FAR, np.int16)
    img[T - 2:T + 2, T - 2:T + 2] = 7
    img[T - 1:T + 1, T - 1:T + 1] = FAR
    return img


def straddlers(T, size):
    """bars of `size` and `size + 1` pixels across the vertical tile edge x = T, and two more across the horizontal edge y = T"""
    img = np.full((2 * T + 3, 2 * T + 3), FAR, np.int16)
    half = size // 2
    img[3, T - half:T - half + size] = 5
    img[9, T - half:T - half + size + 1] = 5
    img[T - half:T - half + size, 4] = 5
    img[T - half:T - half + size + 1, 11] = 5
    return img


def _case(cid, image, new_val, max_size, max_diff):
    return dict(id=cid, image=image, new_val=new_val, max_size=max_size, max_diff=max_diff)


def cases(T):
    out = []
    for w, h in ((1, 1), (1, 37), (37, 1), (T, T), (T + 1, T + 1), (2 * T + 1, T - 1)):
        out.append(_case(f"size_{w}x{h}", lambda w=w, h=h: noise(h, w, (7, 8, 20), 10 + w + h, holes=0.05), -16, min(3, w * h), 0))
    W, H = 3 * T + 1, 2 * T + 1
    length = serpentine(H, W)[1]
    out.append(_case("serpentine_below", lambda: serpentine(H, W)[0], -16, length - 1, 0))
    out.append(_case("serpentine_at", lambda: serpentine(H, W)[0], -16, length, 0))
    out.append(_case("constant_kept", lambda: np.full((H, W), 320, np.int16), -16, 100, 2))
    out.append(_case("constant_removed", lambda: np.full((H, W), 320, np.int16), -16, W * H, 2))
    out.append(_case("all_new_val", lambda: np.full((H, W), -16, np.int16), -16, 100, 2))
    out.append(_case("ring_kept", lambda: ring(T), -16, 11, 0))
    out.append(_case("ring_removed", lambda: ring(T), -16, 12, 0))
    out.append(_case("straddlers", lambda: straddlers(T, 6), -16, 6, 1))
    for md in (0, 1):
        out.append(_case(f"noise_diff{md}", lambda: noise(T + 9, 2 * T + 5, (7, 8, 20), 3, holes=0.03), -16, 4, md))
    out.append(_case("new_val_inside", lambda: noise(T + 3, T + 7, (7, 8, 9), 4), 8, 5, 1))
    for md in (65534, 65535):
        out.append(_case(f"extremes_{md}", lambda: noise(T + 2, T + 5, (32767, -32767, -32768), 5), 0, 3, md))
    return out


_expected = {}


def expected(case):
    """the restatement's result of a case, computed once per process and shared: read-only"""
    if case["id"] not in _expected:
        out = R.filter_speckles(case["image"](), case["new_val"], case["max_size"], case["max_diff"])
        out.setflags(write=False)
        _expected[case["id"]] = out
    return _expected[case["id"]]


def host_filter(img, new_val, max_size, max_diff):
    """vp_filter_speckles_host on a packed array, into a new one"""
    from vision import _vp
    img = np.ascontiguousarray(img)
    h, w = img.shape
    out = np.empty((h, w), np.int16)
    _vp.check(_vp.lib().vp_filter_speckles_host(img.ctypes.data, 2 * w, w, h, int(new_val), int(max_size), int(max_diff), out.ctypes.data, 2 * w))
    return out
