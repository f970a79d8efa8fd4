"""bench.py --dump-outputs: the whole frame as (H, W, 3) in its own dtype while it fits the size limit, else the
pixels at a fixed seeded sample of linear indices -- the same indices in every run, so two builds' dumps of the
same config compare pixel for pixel."""
import os

import numpy as np
import pytest
import torch

import bench


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_whole_frame_keeps_shape_and_dtype(tmp_path, dtype):
    W, H = 7, 5
    fb = torch.arange(W * H * 3, dtype=dtype).reshape(W * H, 3)
    bench.dump_outputs(str(tmp_path / "d"), fb, W, H)
    a = np.load(tmp_path / "d" / "framebuffer.npy")
    assert a.shape == (H, W, 3) and a.dtype == fb.numpy().dtype
    assert (a.reshape(-1, 3) == fb.numpy()).all()


def test_large_frame_is_a_fixed_sample_within_the_limit(tmp_path, monkeypatch):
    W, H = 64, 48
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1000 * 3 * 8)  # 1000 fp64 pixels of the 3072
    fb = torch.arange(W * H * 3, dtype=torch.float64).reshape(W * H, 3)
    bench.dump_outputs(str(tmp_path / "a"), fb, W, H)
    bench.dump_outputs(str(tmp_path / "b"), fb + 0.5, W, H)
    a = np.load(tmp_path / "a" / "framebuffer.npy")
    b = np.load(tmp_path / "b" / "framebuffer.npy")
    assert a.shape == (1000, 3) and a.dtype == np.float64
    assert os.path.getsize(tmp_path / "a" / "framebuffer.npy") <= 1000 * 3 * 8 + 128
    idx = (a[:, 0] / 3).astype(np.int64)  # pixel i holds 3i, 3i+1, 3i+2
    assert (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < W * H
    assert (b == a + 0.5).all()  # the second dump sampled the same pixels
