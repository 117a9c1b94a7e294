"""CPU: bench.py's options and its --dump-outputs writer (no GPU)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_plain_run_is_the_default_and_steps_are_kept():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_dump_writes_float_arrays_and_fixed_samples(tmp_path):
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (2, 3, 4, 64, 64), generator=g, dtype=torch.uint8)
    views = torch.randn(2, 12, 3, 8, 8, generator=g).half()
    faces = torch.arange(30, dtype=torch.int64).reshape(10, 3)
    arrays = {"views": (views, None), "faces": (faces, None), **bench._frames_arrays(frames)}
    arrays["frames"] = (frames, 5000)                 # smaller cap than the bench's: forces a sample
    files = {}
    for d in ("a", "b"):
        files[d] = bench._dump_outputs(str(tmp_path / d), arrays)
    assert files["a"] == files["b"]
    assert set(files["a"]) == {"views.npy", "faces.npy", "frames_sample.npy", "frames_channel_sums.npy"}
    for name in files["a"]:
        x, y = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y)
    assert np.load(tmp_path / "a" / "views.npy").dtype == np.float32
    assert np.array_equal(np.load(tmp_path / "a" / "views.npy"), views.float().numpy())
    f = np.load(tmp_path / "a" / "faces.npy")
    assert f.dtype == np.float64 and np.array_equal(f, faces.numpy())
    # the sample is the flattened frames at the documented seeded indices
    idx = np.unique(np.random.default_rng(0).integers(0, frames.numel(), 5000))
    s = np.load(tmp_path / "a" / "frames_sample.npy")
    assert np.array_equal(s, frames.numpy().reshape(-1)[idx].astype(np.float32))
    sums = np.load(tmp_path / "a" / "frames_channel_sums.npy")
    assert sums.shape == (2, 3, 4) and np.array_equal(sums, frames.double().sum(dim=(-1, -2)).numpy())


def test_dump_stays_under_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1000)
    try:
        bench._dump_outputs(str(tmp_path), {"x": (torch.zeros(1000), None)})
    except ValueError:
        return
    raise AssertionError("an output above the limit was written")


def test_mesh_summary_has_a_fixed_shape():
    class P:
        last_mesh_post = {"verts": np.array([[0.0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 2]]),
                          "faces": np.array([[0, 1, 2], [0, 1, 3]], np.int64),
                          "colors": np.array([[1.0, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]], np.float32)}
    s = dict(zip(bench.MESH_SUMMARY_FIELDS, bench._mesh_summary(P())))
    assert (s["n_verts"], s["n_faces"], s["median_x"], s["median_z"]) == (4, 2, 0.0, 0.0)
    assert abs(s["p95_x"] - 1.7) < 1e-12 and (s["p05_y"], s["mean_color_r"]) == (0.0, 0.5)

    class Empty:
        last_mesh_post = {"verts": np.zeros((0, 3)), "faces": np.zeros((0, 3), np.int64), "colors": None}
    for p in (Empty(), object()):
        z = bench._mesh_summary(p)
        assert z.shape == (len(bench.MESH_SUMMARY_FIELDS),) and not z.any()
