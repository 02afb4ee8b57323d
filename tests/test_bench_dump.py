"""CPU suite: what `bench.py --dump-outputs DIR` writes - one .npy per output in float32 where every value is exact in it, else
float64; an image of the batch as its first and last frame whole plus a seeded sample of the whole batch; the same files from the same
arrays; never more than 64 MB."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def _outputs():
    g = torch.Generator().manual_seed(0)
    B, H, W = 5, 1080, 1920
    return {"threshed": (torch.randint(0, 2, (B, H, W), generator=g) * 255).to(torch.uint8),
            "labels": torch.randint(0, 300, (B, H, W), generator=g, dtype=torch.int32),
            "stats": torch.randint(0, 1 << 20, (B, 256, 5), generator=g, dtype=torch.int32),
            "centroids": torch.rand((B, 256, 2), generator=g, dtype=torch.float64),
            "nlabels": torch.tensor([1, 2, 3, 4, 1 << 24], dtype=torch.int32)}


def test_files_dtypes_and_selection(tmp_path):
    outs = _outputs()
    written = bench.dump_outputs(str(tmp_path), outs)
    assert sorted(written) == sorted(os.listdir(tmp_path)) == ["centroids.npy", "labels_frames.npy", "labels_sample.npy", "nlabels.npy",
                                                                "stats.npy", "threshed_frames.npy", "threshed_sample.npy"]
    assert sum(written.values()) <= bench.DUMP_LIMIT_BYTES
    ld = {f[:-4]: np.load(tmp_path / f) for f in written}
    for name in ("threshed", "labels"):
        a = outs[name].numpy()
        assert ld[name + "_frames"].dtype == np.float32 and np.array_equal(ld[name + "_frames"], a[[0, len(a) - 1]])
        pos = bench.sample_positions(a.size)
        assert len(pos) == bench.DUMP_SAMPLE and np.all(np.diff(pos) > 0) and np.array_equal(pos, bench.sample_positions(a.size))
        assert ld[name + "_sample"].dtype == np.float32 and np.array_equal(ld[name + "_sample"], a.reshape(-1)[pos])
    assert ld["stats"].dtype == np.float32 and np.array_equal(ld["stats"], outs["stats"].numpy())
    assert ld["centroids"].dtype == np.float64 and np.array_equal(ld["centroids"], outs["centroids"].numpy())
    assert ld["nlabels"].dtype == np.float64 and np.array_equal(ld["nlabels"], outs["nlabels"].numpy())   # 2^24 is not exact in float32


def test_same_arrays_same_files(tmp_path):
    outs = _outputs()
    bench.dump_outputs(str(tmp_path / "a"), outs)
    bench.dump_outputs(str(tmp_path / "b"), outs)
    for f in os.listdir(tmp_path / "a"):
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f


def test_over_the_limit_is_an_error(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 10**6)
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path), _outputs())
