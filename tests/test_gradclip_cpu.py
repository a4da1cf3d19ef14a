"""Global-norm gradient clipping without a GPU: the torch twin of the device rule (ops/gradclip.py)
against ``torch.nn.utils.clip_grad_norm_``, its coefficient cases, the config key, the engine's
records on the CPU MLP task and two gloo ranks."""
import json
import math
import os

import numpy as np
import pytest
import torch

from network_distributed_pytorch_amd import engine, ops
from network_distributed_pytorch_amd.ops.gradclip import GradClip
from network_distributed_pytorch_amd.utils.config import ConfigError, validate_config
from network_distributed_pytorch_amd.utils.launcher import spawn

from . import gradclip_dist_helpers as H


def _ulp(x: float) -> float:
    return float(np.spacing(np.float32(abs(x))))


def _torch_clip(tensors, max_norm):
    """torch.nn.utils.clip_grad_norm_ on fp64 copies: (norm, clipped copies)."""
    ps = [torch.nn.Parameter(t.double().clone()) for t in tensors]
    for p, t in zip(ps, tensors):
        p.grad = t.double().clone()
    norm = torch.nn.utils.clip_grad_norm_(ps, max_norm, error_if_nonfinite=False)
    return float(norm), [p.grad for p in ps]


def _tensors(seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) * scale for s in ((7, 5), (33,), (4, 3, 3, 3), (1,), (2049,))]


@pytest.mark.parametrize("max_norm", [0.5, 10.0, 1e4])
def test_twin_matches_torch_clip_grad_norm(max_norm):
    ts = _tensors()
    ref_norm, ref = _torch_clip(ts, max_norm)
    got = [t.clone() for t in ts]
    norm = ops.clip_grad_norm_(got, max_norm)
    assert norm.dtype == torch.float32 and norm.dim() == 0
    assert abs(float(norm) - ref_norm) <= _ulp(ref_norm)
    for a, b in zip(got, ref):
        assert torch.allclose(a.double(), b, rtol=1e-6, atol=0)
    if max_norm == 1e4:  # under the threshold: untouched
        assert all(torch.equal(a, t) for a, t in zip(got, ts))


def test_twin_div_and_block():
    ts = _tensors(1)
    clip = GradClip("cpu")
    clip.bind(ts)
    ref = math.sqrt(sum(float(t.double().pow(2).sum()) for t in ts)) / 3.0
    clip.run(float("inf"), div=3.0)
    st = clip.read()
    assert abs(st["norm"] - ref) <= _ulp(ref) and st["coef"] == 1.0 and st["steps"] == 1 and st["clipped"] == 0
    clip.run(ref / 2, div=3.0)
    st = clip.read()
    assert st["steps"] == 2 and st["clipped"] == 1
    coef = np.float32(ref / 2) / (np.float32(st["norm"]) + np.float32(1e-6))
    assert st["coef"] == float(coef) and st["coef"] < 1.0


def test_twin_coefficient_cases():
    ts = _tensors(2)
    ts[0][0, 0] = -0.0
    keep = [t.clone() for t in ts]
    norm = ops.clip_grad_norm_(ts, float("inf"))
    assert float(norm) > 0 and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(ts, keep))

    zeros = [torch.zeros(5), torch.zeros(0), torch.zeros(3, 3)]
    clip = GradClip("cpu")
    clip.bind(zeros)
    clip.run(1.0)
    assert clip.read()["norm"] == 0.0 and clip.read()["coef"] == 1.0
    empty = GradClip("cpu")
    empty.bind([])
    empty.run(1.0)
    assert empty.read() == {"norm": 0.0, "coef": 1.0, "clipped": 0, "steps": 0}

    bad = _tensors(3)
    bad[2].view(-1)[5] = float("nan")
    clip.bind(bad)
    clip.run(1.0)
    st = clip.read()
    assert math.isnan(st["norm"]) and math.isnan(st["coef"])
    assert all(torch.isnan(t).all() for t in bad)

    big = [torch.tensor([1e25, 3.0]), torch.tensor([-1e25])]
    norm = ops.clip_grad_norm_(big, float("inf"))
    ref = math.sqrt(2.0) * 1e25
    assert math.isfinite(float(norm)) and abs(float(norm) - ref) <= _ulp(ref)


def test_bad_arguments():
    with pytest.raises(ValueError):
        ops.clip_grad_norm_([torch.ones(3)], 0.0)
    with pytest.raises(ValueError):
        ops.clip_grad_norm_([torch.ones(3)], float("nan"))
    with pytest.raises(ValueError):
        ops.clip_grad_norm_([torch.ones(3)], 1.0, div=0.5)


def test_config_key():
    validate_config(engine.default_config())
    assert engine.default_config()["max_grad_norm"] == 0.0
    validate_config(engine.default_config(max_grad_norm=float("inf")))
    validate_config(engine.default_config(max_grad_norm=1.0, grad_sync="dense", overlap=True))
    for bad in (-1.0, float("nan")):
        with pytest.raises(ConfigError):
            validate_config(engine.default_config(max_grad_norm=bad))
    with pytest.raises(ConfigError, match="overlap"):
        validate_config(engine.default_config(max_grad_norm=1.0, grad_sync="powersgd", overlap=True))


def test_cli_flag():
    from network_distributed_pytorch_amd.workloads import _cli

    assert _cli.build_parser(1).parse_args(["-max_grad_norm", "inf"]).max_grad_norm == float("inf")
    assert _cli.build_parser(1).parse_args([]).max_grad_norm is None


def test_powersgd_overlap_with_clip_raises():
    from network_distributed_pytorch_amd.parallel.powersgd import PowerSGDOptimizer

    model = torch.nn.Linear(4, 3)
    with pytest.raises(ValueError, match="overlap.*max_grad_norm"):
        PowerSGDOptimizer(model.parameters(), lr=0.1, rank=2, overlap=True, max_grad_norm=1.0)
    opt = PowerSGDOptimizer(model.parameters(), lr=0.1, rank=2, max_grad_norm=1.0)
    assert opt.overlap is False
    with pytest.raises(ValueError, match="overlap.*max_grad_norm"):
        opt.set_overlap(True)


# ---- the engine on the CPU MLP task --------------------------------------------------------------
def _run(tmp_path, name, grad_sync, max_grad_norm):
    cfg = engine.default_config(task="mlp", grad_sync=grad_sync, dataset_size=256, global_batch=32,
                                training_epochs=1, verbose=False, learning_rate=0.05, max_grad_norm=max_grad_norm,
                                log_file=str(tmp_path / f"{name}.jsonl"))
    torch.manual_seed(1)
    out = engine.run_task(cfg)
    recs = [json.loads(ln) for ln in (tmp_path / f"{name}.jsonl").read_text().splitlines()]
    return out, recs


@pytest.mark.parametrize("grad_sync", ["powersgd", "dense", "powersgd-ref", "dense-ref", "local-sgd-nesterov"])
def test_engine_clip_records_and_effect(tmp_path, grad_sync):
    off, recs_off = _run(tmp_path, "off", grad_sync, 0.0)
    assert not any(k in r for r in recs_off for k in ("grad_norm", "clip_coef", "clipped_steps", "max_grad_norm"))
    assert "clipped_steps" not in off

    inf, recs = _run(tmp_path, "inf", grad_sync, float("inf"))
    for a, b in zip(off["model"].parameters(), inf["model"].parameters()):
        assert torch.equal(a, b)
    steps = [r for r in recs if r["kind"] == "step"]
    assert [r["loss"] for r in steps] == [r["loss"] for r in recs_off if r["kind"] == "step"]
    assert len(steps) == 8 and all(r["grad_norm"] > 0 and r["clip_coef"] == 1.0 for r in steps)
    assert inf["clipped_steps"] == 0 and recs[-1]["clipped_steps"] == 0 and recs[-1]["max_grad_norm"] == float("inf")
    assert [r["clipped_steps"] for r in recs if r["kind"] == "epoch"] == [0]

    norms = [r["grad_norm"] for r in steps]
    lo, hi = min(norms), max(norms)
    assert lo < hi
    thr = float(np.float32(0.5 * (lo + hi)))
    assert lo < thr < hi
    cl, recs_c = _run(tmp_path, "clip", grad_sync, thr)
    assert 0 < cl["clipped_steps"] < len(steps)
    csteps = [r for r in recs_c if r["kind"] == "step"]
    assert sum(r["clip_coef"] != 1.0 for r in csteps) == cl["clipped_steps"]
    assert any(not torch.equal(a, b) for a, b in zip(off["model"].parameters(), cl["model"].parameters()))


# ---- two gloo ranks ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "powersgd"])
def test_two_ranks_stay_identical_under_clipping(tmp_path, kind):
    spawn(H.clip_rank_body, 2, args=(str(tmp_path), kind, 0.05, 3))
    a, b = (torch.load(os.path.join(tmp_path, f"{kind}_rank{r}.pt"), weights_only=True) for r in range(2))
    for p, q in zip(a["params"], b["params"]):
        assert torch.equal(p, q)
    assert [s["steps"] for s in a["stats"]] == [1, 2, 3]
    assert a["stats"][-1]["clipped"] == 3 and b["stats"][-1]["clipped"] == 3  # the threshold bites every step
    na, nb = [s["norm"] for s in a["stats"]], [s["norm"] for s in b["stats"]]
    if kind == "dense":  # the norm of the averaged gradient: the same number on both ranks
        assert na == nb
    else:                # each rank clips its own gradient by its own norm
        assert all(x != y for x, y in zip(na, nb))
