"""Depth images for the surface-normal tests, and the host routine on packed arrays."""
import numpy as np


def wall(h, w, z=2.0):
    return np.full((h, w), z, np.float32)


def tilted_plane(h, w, f, z0=3.0, about="vertical", degrees=20.0, cx=None, cy=None):
    """float32 depth of the plane through (0, 0, z0) whose normal towards the camera is (sin a, 0, -cos a) (about the vertical axis) or
    (0, sin a, -cos a) (about the horizontal one): Z = z0 / (1 - tan a * u), u = (x - cx) / f or (y - cy) / f.  Returns depth and normal."""
    a = np.deg2rad(degrees)
    cx = (w - 1) / 2 if cx is None else cx
    cy = (h - 1) / 2 if cy is None else cy
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    u = (x - cx) / f if about == "vertical" else (y - cy) / f
    z = z0 / (1.0 - np.tan(a) * u)
    n = (np.sin(a), 0.0, -np.cos(a)) if about == "vertical" else (0.0, np.sin(a), -np.cos(a))
    return z.astype(np.float32), np.array(n)


def noisy_depth(h, w, seed=0):
    """a slanted surface under noise, with holes of every unusable kind: 0, negative, NaN, +inf"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    z = (2.0 + 0.01 * x + 0.02 * y + rng.normal(0, 0.05, (h, w))).astype(np.float32)
    kinds = np.array([0.0, -1.0, np.nan, np.inf], np.float32)
    holes = rng.random((h, w)) < 0.06
    z[holes] = kinds[rng.integers(0, 4, int(holes.sum()))]
    return z


def host_normals(depth, f, cx=None, cy=None, max_jump_m=None, encode=False, zpad=0, npad=0):
    """vp_normals_from_depth_host; zpad / npad: extra floats at the end of every row of the depth / the result (which must come back
    untouched)"""
    from vision import _vp
    h, w = depth.shape
    zbuf = np.full((h, w + zpad), 777.0, np.float32)
    zbuf[:, :w] = depth
    nbuf = np.full((h, 3 * w + npad), -5.0, np.float32)
    _vp.check(_vp.lib().vp_normals_from_depth_host(zbuf.ctypes.data, 4 * (w + zpad), w, h, float(f), float((w - 1) / 2 if cx is None else cx),
                                                   float((h - 1) / 2 if cy is None else cy), 0.0 if max_jump_m is None else float(max_jump_m), int(encode),
                                                   nbuf.ctypes.data, 4 * (3 * w + npad)))
    assert np.all(nbuf[:, 3 * w:] == -5.0), "the result's padding was written"
    return np.ascontiguousarray(nbuf[:, :3 * w]).reshape(h, w, 3)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
