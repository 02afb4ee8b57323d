"""The inputs of the colour-balance GPU tests, checked with the oracle alone: the tiled frames of balance_cases must make the
reference keep the tiles' own means (cpp:474 replaces a tile's means by the global ones when one of them is more than 1/6 away), or
a kernel that gave every tile the global gains would pass the GPU tests for lack of signal."""
import numpy as np
import pytest

import balance_cases as BC

CASES = BC.tiled_cases()


def test_the_cases_are_the_ones_the_kernels_need():
    """Tile widths that are no multiple of 4, widths and pixel counts that are no multiple of 4, one-pixel tiles, 63 tiles at most."""
    assert len(CASES) == 9
    geo = [(f.shape[0], f.shape[1], hb, vb) for _, f, hb, vb in CASES]
    assert any((w // hb) % 4 for h, w, hb, vb in geo) and any(w % 4 for h, w, hb, vb in geo) and any((h * w) % 4 for h, w, hb, vb in geo)
    assert any(w // hb == 1 and h // vb == 1 for h, w, hb, vb in geo)
    assert all(w % hb == 0 and h % vb == 0 and max(h, w) <= 45 for h, w, hb, vb in geo)
    fr = BC.batch_frames()
    assert fr.shape == (3, 30, 40, 3) and fr.dtype == np.uint8 and fr[0].size % 4 == 0
    assert not np.array_equal(fr[0], fr[1]) and not np.array_equal(fr[1], fr[2]) and not np.array_equal(fr[0], fr[2])
    assert all(40 % hb == 0 and 30 % vb == 0 for hb, vb in BC.BATCH_TILINGS)


@pytest.mark.parametrize("name,frame,hb,vb", CASES, ids=[c[0] for c in CASES])
def test_tiles_keep_their_own_means_in_the_oracle(oracle, name, frame, hb, vb):
    """With the HSV stage off a tile whose means were replaced by the global ones equals the 1 x 1 result exactly.  So the tiled result
    must differ from the 1 x 1 result inside at least three quarters of the tiles, and two tiles must map one input value of one channel
    to different outputs (with the HSV stage off a channel's output is a function of the tile and the channel's input value alone)."""
    h, w, _ = frame.shape
    tiled = oracle.color_balance(frame, horizontal_blocks=hb, vertical_blocks=vb, hsv_contrast_correct=False, mean_mode=0)
    whole = oracle.color_balance(frame, horizontal_blocks=1, vertical_blocks=1, hsv_contrast_correct=False, mean_mode=0)
    tile = BC.tile_index(h, w, hb, vb)
    differs = (tiled != whole).any(axis=2)
    kept = np.unique(tile[differs]).size
    assert 4 * kept >= 3 * hb * vb, (name, kept, hb * vb)
    for c in range(3):
        seen = {}
        for t, v, o in zip(tile.ravel().tolist(), frame[:, :, c].ravel().tolist(), tiled[:, :, c].ravel().tolist()):
            first = seen.setdefault(v, (t, o))
            if first[0] != t and first[1] != o:
                return
    raise AssertionError((name, "no input value is mapped differently by two tiles"))


def test_the_oracle_accepts_every_small_frame_case(oracle):
    """test_small_frames (GPU) leaves out the flag sets the oracle rejects at 1 to 7 pixels: there are none."""
    import frames as F
    from test_gpu_balance import FLAG_SETS
    for h, w in BC.SMALL_FRAMES:
        for flags in FLAG_SETS:
            out = oracle.color_balance(F.s3_noise(0, w, h), mean_mode=0, **flags)
            assert out.shape == (h, w, 3) and out.dtype == np.uint8, (h, w, flags)
