"""bench.py --dump-outputs / --full on CPU: the flags parse, a plain run asks for no extra arm,
and dump_outputs writes the whole arrays under the byte budget and the same seeded sample of
them above it."""
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_dump_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _workload(seed=0):
    torch.manual_seed(seed)
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3), torch.nn.BatchNorm2d(8), torch.nn.Linear(5, 7))
    return types.SimpleNamespace(model=model, loss_acc=torch.tensor(12.5))


def test_flags_parse_and_plain_run_has_no_extra_arm(bench):
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    assert a.weak_too == "off" and a.link == "none" and a.amp == "none"
    b = bench.parse(["--full", "--dump-outputs", "out"])
    assert b.full is True and b.dump_outputs == "out"


def test_dump_outputs_whole(bench, tmp_path):
    wl = _workload()
    written = bench.dump_outputs(wl, str(tmp_path / "d"), 2.5)
    params = np.load(tmp_path / "d" / "params.npy")
    buffers = np.load(tmp_path / "d" / "buffers.npy")
    loss = np.load(tmp_path / "d" / "loss.npy")
    want = torch.cat([p.detach().reshape(-1) for p in wl.model.parameters()]).numpy()
    assert params.dtype == np.float32 and np.array_equal(params, want)
    assert buffers.dtype == np.float32 and buffers.size == 8 + 8 + 1
    assert loss.dtype == np.float64 and loss.tolist() == [2.5, 12.5]
    assert written == {"params": want.size, "buffers": 17, "loss": 2}


def test_dump_outputs_sample_is_fixed_and_within_budget(bench, tmp_path, monkeypatch):
    wl = _workload()
    want = torch.cat([p.detach().reshape(-1) for p in wl.model.parameters()]).numpy()
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * (want.size + 17) // 3)
    bench.dump_outputs(wl, str(tmp_path / "a"), 0.0)
    bench.dump_outputs(wl, str(tmp_path / "b"), 0.0)
    a, b = np.load(tmp_path / "a" / "params.npy"), np.load(tmp_path / "b" / "params.npy")
    assert np.array_equal(a, b) and 0 < a.size <= want.size // 3 + 1
    nbytes = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert nbytes <= 4 * (want.size + 17) // 3 + 3 * 128 + 16  # .npy headers + the loss pair
    # the sample is a subsequence of the whole array (index order kept)
    it = iter(want.tolist())
    assert all(any(v == w for w in it) for v in a.tolist())
