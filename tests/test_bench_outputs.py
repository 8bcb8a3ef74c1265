"""bench.py --dump-outputs without a GPU: dump_outputs() on host tensors shaped like one step's maps of the bench view."""
import numpy as np
import pytest
import torch

import bench


def _outputs(seed, n=262144, samples=64):
    g = torch.Generator().manual_seed(seed)
    return {"rgb_map": torch.rand((1, n, 3), generator=g), "acc_map": torch.rand((1, n), generator=g),
            "depth_map": torch.rand((1, n), generator=g, dtype=torch.float64),
            # weights[0, r, 0] = r names the ray a sampled row came from
            "weights": torch.cat([torch.arange(n, dtype=torch.float32).reshape(1, n, 1), torch.rand((1, n, samples - 1), generator=g)], 2)}


def test_dump_outputs_writes_every_map_within_the_budget(tmp_path):
    outs = _outputs(0)
    bench.dump_outputs(str(tmp_path), outs)
    names = sorted(p.name for p in tmp_path.iterdir())
    assert names == ["acc_map.npy", "depth_map.npy", "rgb_map.npy", "weights_sample.npy"]
    assert sum(p.stat().st_size for p in tmp_path.iterdir()) <= bench.DUMP_MAX_BYTES + 4096
    rgb = np.load(str(tmp_path / "rgb_map.npy"))
    assert rgb.dtype == np.float32 and np.array_equal(rgb, outs["rgb_map"].numpy())
    depth = np.load(str(tmp_path / "depth_map.npy"))
    assert depth.dtype == np.float64 and np.array_equal(depth, outs["depth_map"].numpy())
    w = np.load(str(tmp_path / "weights_sample.npy"))
    assert w.dtype == np.float32 and w.shape[0] == 1 and w.shape[2] == 64 and 0 < w.nbytes <= bench.DUMP_SAMPLE_BYTES
    # the sample is a set of whole rays, each row equal to one row of the full array
    full = outs["weights"].numpy()[0]
    rows = w[0, :, 0].astype(np.int64)
    assert np.all(np.diff(rows) > 0) and np.array_equal(full[rows], w[0])


def test_dump_outputs_samples_the_same_rays_every_run(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), _outputs(1))
    bench.dump_outputs(str(b), _outputs(1))
    for name in ("rgb_map.npy", "weights_sample.npy"):
        assert np.array_equal(np.load(str(a / name)), np.load(str(b / name)))


def test_dump_outputs_refuses_more_than_the_budget(tmp_path):
    many = {"map%d" % i: torch.zeros((1, 1 << 20, 4)) for i in range(5)}  # 5 x 16 MB, each just at the sampling threshold
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path), many)
    assert not tmp_path.exists() or not any(tmp_path.iterdir())
