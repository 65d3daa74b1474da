"""bench.py --dump-outputs (``bench.dump_outputs``) on host tensors: the files it writes, float32, an array
over the per-array limit written as the same seeded sample in every call, and --full / --dump-outputs parsed."""
import os
import sys

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def bench():
    """bench.py as a module; the MIOpen settings its import puts into the environment are taken out again."""
    import importlib
    saved = dict(os.environ)
    try:
        return importlib.import_module("bench")
    finally:
        os.environ.clear()
        os.environ.update(saved)


def test_dump_outputs_files_and_sample(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_ARRAY_BYTES", 4 * 1000)
    torch.manual_seed(0)
    net = torch.nn.Linear(7, 3)
    loss = torch.tensor(0.25, dtype=torch.float64)
    big = torch.arange(5000, dtype=torch.float32).reshape(50, 100)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), loss, big, {"model": net})
    assert sorted(os.listdir(tmp_path / "a")) == ["filtered.npy", "params_model.npy", "returned_0.npy"]
    a = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    b = {f: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    for f in a:
        assert a[f].dtype == np.float32 and np.array_equal(a[f], b[f])
    assert a["returned_0.npy"].tolist() == [0.25]
    want = torch.cat([p.detach().reshape(-1) for p in net.parameters()]).numpy()
    assert np.array_equal(a["params_model.npy"], want)
    s = a["filtered.npy"]  # 1000 of 5000 elements, values are their own flat indices
    assert s.shape == (1000,) and np.all(np.diff(s) >= 0) and s.min() >= 0 and s.max() < 5000
    assert len(np.unique(s)) > 800  # drawn over the whole array, not one corner
    assert s.max() - s.min() > 4000


def test_dump_outputs_returned_batch_written_once(bench, tmp_path):
    y = torch.ones(2, 3)
    bench.dump_outputs(str(tmp_path), y, y, {})
    assert os.listdir(tmp_path) == ["returned_0.npy"]
    assert np.load(tmp_path / "returned_0.npy").shape == (6,)


def test_parse_full_off_by_default(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "1"])
    a = bench.parse()
    assert not a.full and a.no_cpu_baseline and a.dump_outputs is None and a.steps == 4
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and not a.no_cpu_baseline and a.dump_outputs == "out"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu-baseline"])
    assert bench.parse().no_cpu_baseline
