"""bench.py --dump-outputs on the CPU: the writer keeps whole arrays (float32) while they fit
the budget and cuts them to the same seeded sample on every call once they do not; a plain
command line switches every side row off and --full leaves them on."""
import os
import sys

import numpy as np
import torch

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _REPO)
import bench  # noqa: E402


def _tensors():
    g = torch.Generator().manual_seed(7)
    return {"O": torch.rand((2, 3, 50, 8), generator=g), "L": torch.rand((2, 3, 50), generator=g).half()}


def test_dump_whole_arrays(tmp_path):
    t = _tensors()
    bench.dump_outputs(str(tmp_path / "d"), t)
    for name, x in t.items():
        a = np.load(tmp_path / "d" / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == tuple(x.shape)
        assert np.array_equal(a, x.float().numpy())


def test_dump_sample_is_bounded_and_repeatable(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * 300)
    t = _tensors()
    bench.dump_outputs(str(tmp_path / "a"), t)
    bench.dump_outputs(str(tmp_path / "b"), t)
    total = 0
    for name, x in t.items():
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and a.ndim == 1 and 0 < a.size < x.numel()
        assert np.array_equal(a, b)
        assert np.isin(a, x.float().numpy()).all()
        total += a.nbytes
    assert total <= 4 * 300


def test_plain_run_switches_side_rows_off(monkeypatch):
    flags = ("no_int8", "no_cpu", "no_c5", "no_mla", "no_sparse", "no_next", "no_strong")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    args = bench.parse()
    assert not args.full and args.steps == 3 and all(getattr(args, f) for f in flags)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu"])
    args = bench.parse()
    assert args.full and args.no_cpu and not any(getattr(args, f) for f in flags if f != "no_cpu")
