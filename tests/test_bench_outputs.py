"""bench.py --dump-outputs on the host (no GPU): the 64 MB cap and the seeded pixel sample of a frame that exceeds it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_fit_64_mb_with_the_same_sample_every_time(tmp_path):
    H, W = 1080, 1920                     # config #4's frame: 44 B per pixel over three arrays, 91 MB
    idx = np.arange(H * W, dtype=np.float32).reshape(H, W, 1)          # (every channel holds its pixel's index)
    frame = {"image": np.repeat(idx, 3, -1), "vpl_accum": np.repeat(idx, 4, -1), "photon_accum": np.repeat(idx, 4, -1)}
    info = bench.write_outputs(np, str(tmp_path / "a"), frame)
    bench.write_outputs(np, str(tmp_path / "b"), frame)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert sorted(os.listdir(tmp_path / "a")) == ["image.npy", "photon_accum.npy", "vpl_accum.npy"]
    assert 0.95 * bench.DUMP_BYTES < total <= bench.DUMP_BYTES and info["pixels"] != "all"
    pixels = None
    for k, v in frame.items():
        a, b = np.load(tmp_path / "a" / (k + ".npy")), np.load(tmp_path / "b" / (k + ".npy"))
        assert a.dtype == np.float32 and a.shape[1] == v.shape[-1] and list(a.shape) == info["arrays"][k]
        assert a.tobytes() == b.tobytes()
        assert (a == a[:, :1]).all() and (np.diff(a[:, 0]) > 0).all()     # whole pixels, in image order, none twice
        if pixels is None:
            pixels = a[:, 0]
        assert np.array_equal(a[:, 0], pixels)                              # the same pixels in every array


def test_dump_outputs_write_a_small_frame_whole(tmp_path):
    img = np.random.default_rng(1).random((48, 64, 3), dtype=np.float32)
    info = bench.write_outputs(np, str(tmp_path), {"image": img})
    assert info["pixels"] == "all" and info["arrays"] == {"image": [48, 64, 3]}
    assert np.load(tmp_path / "image.npy").tobytes() == img.tobytes()
