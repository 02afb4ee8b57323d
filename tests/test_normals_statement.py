"""CPU suite for the surface normals' statement: tests/normals_restate.py on depth images with known answers, and
vp_normals_from_depth_host (the same statement as scalar C++) equal to it bit for bit."""
import numpy as np
import pytest

import normals_cases as NC
import normals_restate as R


def _both(depth, f, **kw):
    want = R.normals_from_depth(depth, f, **kw)
    got = NC.host_normals(depth, f, **kw)
    assert want.dtype == np.float32 and want.shape == depth.shape + (3,)
    assert NC.same_bits(got, want), f"the host routine differs from the statement in {int((got.view(np.uint32) != want.view(np.uint32)).sum())} floats"
    return want


def test_a_wall_square_to_the_axis():
    depth = NC.wall(5, 7)
    raw = _both(depth, 500.0)
    assert np.all(raw[1:-1, 1:-1] == np.array([0.0, 0.0, -1.0], np.float32))
    enc = _both(depth, 500.0, encode=True)
    assert np.all(enc[1:-1, 1:-1] == np.array([0.5, 0.5, 0.0], np.float32))
    # an off-centre principal point changes nothing for a wall
    assert np.all(_both(depth, 321.5, cx=1.25, cy=-3.0)[1:-1, 1:-1] == np.array([0.0, 0.0, -1.0], np.float32))


@pytest.mark.parametrize("about", ["vertical", "horizontal"])
def test_a_tilted_plane_meets_its_analytic_normal(about):
    """A plane's pixels back-project onto the plane exactly, so only rounding remains - the statement's own in double, and that of the
    float32 depth, 2^-24 relative, which reaches the normal as the difference of two depths (<= 2^-23 Z) over the baseline between the
    two neighbours (2 Z / f): at f = 4 px that is 2^-23 * 4 / 2 = 2.4e-7 per axis, inside the 1e-6 asked for.  (At f = 500 px the float32
    depth alone would cost 3e-5; that is the input's precision, not the operator's.)"""
    f = 4.0
    depth, n = NC.tilted_plane(7, 9, f, about=about)
    got = _both(depth, f)[1:-1, 1:-1].astype(np.float64)
    err = np.abs(got - n).max()
    print(f"tilted about the {about} axis: largest component error {err:.3e}")
    assert err <= 1e-6
    assert np.allclose(np.linalg.norm(got, axis=-1), 1.0, atol=1e-6)
    enc = _both(depth, f, encode=True)[1:-1, 1:-1].astype(np.float64)
    assert np.abs(enc - (n + 1) / 2).max() <= 1e-6


def test_where_there_is_no_normal():
    nan3 = np.full(3, np.nan, np.float32)
    raw = _both(NC.wall(5, 6), 500.0)
    ringmask = np.ones((5, 6), bool)
    ringmask[1:-1, 1:-1] = False
    assert np.all(np.isnan(raw[ringmask])) and not np.any(np.isnan(raw[~ringmask]))          # the border ring
    assert np.all(_both(NC.wall(5, 6), 500.0, encode=True)[ringmask] == 0)
    for bad in (0.0, np.nan, -1.0, np.inf, -np.inf):
        depth = NC.wall(5, 5)
        depth[2, 3] = bad                                                                      # the centre's right neighbour
        raw = _both(depth, 500.0)
        have = ~np.isnan(raw[:, :, 0])
        # (2, 2), (2, 3) itself, (1, 3) and (3, 3) see it; the other five of the inner 3 x 3 do not
        assert have[1:-1, 1:-1].tolist() == [[True, True, False], [True, False, False], [True, True, False]], bad
        assert NC.same_bits(raw[2, 2], nan3)
        assert np.all(_both(depth, 500.0, encode=True)[2, 2] == 0)


def test_the_jump_guard_admits_exactly_max_jump_m():
    depth = NC.wall(3, 3, 2.0)
    depth[1, 2] = 2.5
    assert not np.any(np.isnan(_both(depth, 500.0)[1, 1]))                                    # no guard
    assert not np.any(np.isnan(_both(depth, 500.0, max_jump_m=0.5)[1, 1]))                    # exactly at it
    depth[1, 2] = np.nextafter(np.float32(2.5), np.float32(3))
    assert np.all(np.isnan(_both(depth, 500.0, max_jump_m=0.5)[1, 1]))                        # just over
    assert not np.any(np.isnan(_both(depth, 500.0, max_jump_m=0.0)[1, 1]))                    # <= 0 and infinite: no guard
    assert not np.any(np.isnan(_both(depth, 500.0, max_jump_m=np.inf)[1, 1]))
    depth[1, 2], depth[0, 1] = 2.0, 1.5                                                       # a nearer neighbour counts the same
    assert np.all(np.isnan(_both(depth, 500.0, max_jump_m=0.25)[1, 1]))


def test_sizes_without_an_interior():
    for h, w in ((1, 1), (2, 9), (9, 2), (1, 4)):
        assert np.all(np.isnan(_both(NC.wall(h, w), 500.0)))
        assert np.all(_both(NC.wall(h, w), 500.0, encode=True) == 0)
    one = _both(NC.wall(3, 3), 500.0)
    assert (~np.isnan(one[:, :, 0])).sum() == 1


def test_host_routine_equals_the_statement_bit_for_bit():
    depth = NC.noisy_depth(45, 67, 1)
    for kw in (dict(), dict(encode=True), dict(max_jump_m=0.08), dict(max_jump_m=0.08, encode=True), dict(cx=30.5, cy=20.25)):
        want = _both(depth, 534.48, **kw)
        assert NC.same_bits(NC.host_normals(depth, 534.48, zpad=3, npad=5, **kw), want)
    have = ~np.isnan(R.normals_from_depth(depth, 534.48)[:, :, 0])
    guarded = ~np.isnan(R.normals_from_depth(depth, 534.48, max_jump_m=0.08)[:, :, 0])
    assert 500 < guarded.sum() < have.sum() < 43 * 65                                         # holes bite, and the guard bites further
    plane, _ = NC.tilted_plane(45, 67, 534.48, degrees=35.0)
    _both(plane, 534.48)
    _both(plane, 534.48, encode=True)
