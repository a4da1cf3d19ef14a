"""Learning-rate schedule and weight decay on the CPU: the schedule's closed forms (utils/schedule.py),
the config rules, the torch twins of the update kernels against an fp64 evaluation of the element
rule, and the engine (logged lr, bitwise resume)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from network_distributed_pytorch_amd import engine, ops
from network_distributed_pytorch_amd.parallel.powersgd import PowerSGDOptimizer, orthogonalize
from network_distributed_pytorch_amd.utils.config import ConfigError, validate_config
from network_distributed_pytorch_amd.utils.schedule import LrSchedule, parse_milestones


def _f32(v):
    return float(np.float32(v))


# ---- the schedule ------------------------------------------------------------------------------
def test_warmup_end_points_then_constant():
    s = LrSchedule(0.4, steps_per_epoch=10, epochs=3, warmup_steps=5)
    assert s.lr_at(0) == _f32(0.4 * 1 / 5)
    assert s.lr_at(4) == _f32(0.4)          # the last warm-up step reaches the base rate
    assert [s.lr_at(k) for k in range(5)] == [_f32(0.4 * (k + 1) / 5) for k in range(5)]
    assert s.lr_at(5) == s.lr_at(29) == _f32(0.4)
    assert s.varies and not LrSchedule(0.4, 10, 3).varies


def test_step_milestones_switch_at_epoch_boundaries():
    s = LrSchedule(0.1, steps_per_epoch=7, epochs=6, schedule="step", milestones=[2, 4], gamma=0.1)
    assert s.lr_at(2 * 7 - 1) == _f32(0.1)
    assert s.lr_at(2 * 7) == _f32(0.1 * 0.1)
    assert s.lr_at(4 * 7 - 1) == _f32(0.1 * 0.1)
    assert s.lr_at(4 * 7) == s.lr_at(6 * 7 - 1) == _f32(0.1 * 0.1 ** 2)
    # a milestone at epoch 0 applies from the first step after the warm-up
    z = LrSchedule(0.1, 7, 6, schedule="step", milestones=[0], gamma=0.5, warmup_steps=2)
    assert z.lr_at(1) == _f32(0.1) and z.lr_at(2) == _f32(0.05)


def test_cosine_first_and_last_step_and_floor():
    S, E, W, base, lo = 5, 4, 3, 0.2, 0.01
    s = LrSchedule(base, S, E, schedule="cosine", warmup_steps=W, lr_min=lo)
    T = S * E
    assert s.lr_at(W - 1) == _f32(base)
    assert s.lr_at(W) == _f32(base)  # cos(0) = 1: the cosine starts at the base rate
    last = lo + (base - lo) * 0.5 * (1 + math.cos(math.pi * (T - 1 - W) / (T - W)))
    assert s.lr_at(T - 1) == _f32(last)
    mid = lo + (base - lo) * 0.5 * (1 + math.cos(math.pi * 6 / (T - W)))
    assert s.lr_at(W + 6) == _f32(mid)
    vals = [s.lr_at(k) for k in range(W, T)]
    assert all(a > b for a, b in zip(vals, vals[1:])) and vals[-1] > _f32(lo)
    assert abs(s.lr_at(T) - lo) < 1e-9  # the curve's end point is lr_min (one past the last step)


@pytest.mark.parametrize("kw", [dict(), dict(schedule="cosine", warmup_steps=7, lr_min=1e-3),
                                dict(schedule="step", milestones=[1, 2], gamma=0.3, warmup_steps=3)])
def test_values_are_fp32(kw):
    s = LrSchedule(0.1, 11, 3, **kw)
    for k in range(33):
        v = s.lr_at(k)
        assert isinstance(v, float) and v == float(np.float32(v))
        assert torch.tensor(v, dtype=torch.float32).item() == v


def test_warmup_must_end_before_the_run():
    with pytest.raises(ValueError, match="lr_warmup_steps"):
        LrSchedule(0.1, 4, 2, warmup_steps=8)
    LrSchedule(0.1, 4, 2, warmup_steps=7)


def test_parse_milestones():
    assert parse_milestones("") == [] and parse_milestones("15,25") == [15, 25] and parse_milestones(" 0, 3 ") == [0, 3]
    for bad in ("5,3", "3,3", "a", "-1", "1.5"):
        with pytest.raises(ValueError):
            parse_milestones(bad)


# ---- config ------------------------------------------------------------------------------------
def test_config_defaults_and_cli_flags():
    c = validate_config(engine.default_config())
    assert (c["lr_schedule"], c["lr_warmup_steps"], c["lr_min"], c["lr_milestones"], c["lr_gamma"],
            c["weight_decay"]) == ("constant", 0, 0.0, "", 0.1, 0.0)
    from network_distributed_pytorch_amd.workloads import _cli

    args = _cli.build_parser(1).parse_args(["-lr", "0.1", "-lr_schedule", "cosine", "-lr_warmup_steps", "200",
                                            "-weight_decay", "5e-4", "-lr_min", "1e-4", "-lr_gamma", "0.2"])

    class _Mod:
        config = engine.default_config()
    _cli.apply_args(_Mod, args, 0, 1, None)
    c = validate_config(_Mod.config)
    assert (c["learning_rate"], c["lr_schedule"], c["lr_warmup_steps"], c["weight_decay"], c["lr_min"],
            c["lr_gamma"]) == (0.1, "cosine", 200, 5e-4, 1e-4, 0.2)
    args = _cli.build_parser(1).parse_args(["-lr_schedule", "step", "-lr_milestones", "15,25"])
    _cli.apply_args(_Mod, args, 0, 1, None)
    assert validate_config(_Mod.config)["lr_milestones"] == "15,25"


@pytest.mark.parametrize("bad", [
    dict(weight_decay=-1e-4), dict(lr_min=-0.1), dict(learning_rate=0.1, lr_min=0.2), dict(lr_warmup_steps=-1),
    dict(lr_gamma=0.0), dict(lr_gamma=-0.5), dict(lr_schedule="linear"),
    dict(lr_schedule="step", lr_milestones="5,3"), dict(lr_schedule="step", lr_milestones="3,3"),
    dict(lr_schedule="step", lr_milestones="-1,3"), dict(lr_schedule="step", lr_milestones="a"),
    dict(lr_schedule="cosine", lr_milestones="3"), dict(lr_milestones="3"), dict(lr_warmup_steps=1.5),
])
def test_config_rejects(bad):
    with pytest.raises(ConfigError):
        validate_config(engine.default_config(**bad))


def test_engine_rejects_warmup_not_below_total_steps():
    cfg = engine.default_config(task="mlp", grad_sync="dense-ref", dataset_size=128, global_batch=64,
                                training_epochs=2, lr_warmup_steps=4, verbose=False)
    with pytest.raises(ConfigError, match="lr_warmup_steps"):
        engine.run_task(cfg)


# ---- the torch twins against fp64 --------------------------------------------------------------
def _close(a, b):
    return torch.allclose(a, b.to(a.dtype), atol=1e-5, rtol=1e-4)


def test_sgd_momentum_cpu_weight_decay_matches_fp64():
    gen = torch.Generator().manual_seed(3)
    wd, mu, div = 5e-2, 0.9, 2.0
    x = torch.randn(1023, generator=gen)
    b = torch.zeros(1023)
    x64, b64 = x.double(), b.double()
    for lr in (0.1, 0.4, 0.05):
        g = torch.randn(1023, generator=gen)
        ops.sgd_momentum_(x, g, b, lr, mu, div, weight_decay=wd)
        d = g.double() / div + wd * x64
        b64 = mu * b64 + d
        x64 = x64 - lr * b64
    assert _close(x, x64) and _close(b, b64)
    # torch.optim.SGD(momentum, weight_decay) is the same rule
    p = torch.nn.Parameter(torch.ones(5))
    ref = torch.optim.SGD([p], lr=0.1, momentum=mu, weight_decay=wd)
    xx, bb = torch.ones(5), torch.zeros(5)
    for _ in range(3):
        p.grad = torch.full((5,), 0.25)
        ref.step()
        ops.sgd_momentum_(xx, torch.full((5,), 0.25), bb, 0.1, mu, 1.0, weight_decay=wd)
    assert torch.allclose(xx, p.detach(), atol=1e-6)


def _fp64_powersgd_step(st, grads, lr, wd, lam, rank):
    """One step of the element rule in fp64 on ``st`` = {x, e, m, q}: lists aligned with ``grads``."""
    for i, g in enumerate(grads):
        x, m = st["x"][i], st["m"][i]
        if g.dim() > 1:
            n = g.shape[0]
            M = g.double().reshape(n, -1) + st["e"][i]
            P = orthogonalize(M @ st["q"][i])
            Q = M.t() @ P
            o = P @ Q.t()
            st["e"][i] = M - o
            st["q"][i] = Q
            o = o.reshape(g.shape)
        else:
            o = g.double()
        d = o + wd * x if wd != 0 else o
        m.mul_(lam).add_(d)
        x.sub_(lr * (d + m))


@pytest.mark.parametrize("write_grad", [False, True])
def test_powersgd_torch_twin_weight_decay_matches_fp64(write_grad):
    gen = torch.Generator().manual_seed(11)
    shapes = [(12, 10), (8, 3, 3, 3), (50,), (6, 4)]
    ps = [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in shapes]
    lam, wd, rank = 0.9, 5e-2, 2
    opt = PowerSGDOptimizer(ps, lr=0.1, momentum=lam, rank=rank, native=False, write_grad=write_grad)
    assert not opt.native and opt.hyper is None
    opt.prepare()
    hi = [i for i, s in enumerate(shapes) if len(s) > 1]
    st = {"x": [p.detach().double().clone() for p in ps], "m": [torch.zeros(s, dtype=torch.float64) for s in shapes],
          "e": [torch.zeros(s[0], int(np.prod(s[1:])), dtype=torch.float64) if len(s) > 1 else None for s in shapes],
          "q": [None] * len(shapes)}
    for k, i in enumerate(hi):
        st["q"][i] = opt.buf.q_view(k).double().clone()
    for lr in (0.1, 0.4, 0.05):
        lr = _f32(lr)
        grads = [torch.randn(s, generator=gen) for s in shapes]
        opt.set_hyper(lr, wd)
        assert opt.lr == lr and opt.weight_decay == _f32(wd)
        opt.zero_grad()
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        x_before = [p.detach().double().clone() for p in ps]
        opt.step()
        _fp64_powersgd_step(st, grads, lr, _f32(wd), lam, rank)
        for i, p in enumerate(ps):
            assert _close(p.detach(), st["x"][i]), i
            assert _close(opt._view(opt.m, p).view_as(p), st["m"][i]), i
            if p.dim() > 1:
                assert _close(opt._view(opt.e, p).view(p.shape[0], -1), st["e"][i]), i
            if write_grad:  # grad = d + m', which the parameter step confirms: x' = x - lr grad
                assert _close(p.grad, (x_before[i] - st["x"][i]) / lr), i
    sd = opt.state_dict()
    assert sd["weight_decay"] == _f32(wd) and sd["lr"] == _f32(0.05)
    del sd["weight_decay"]  # a checkpoint from before the key existed
    opt.load_state_dict(sd)
    assert opt.weight_decay == 0.0


# ---- the engine --------------------------------------------------------------------------------
def _cfg(tmp_path, name, **over):
    base = dict(task="mlp", dataset_size=256, global_batch=64, training_epochs=2, verbose=False, learning_rate=0.05,
                lr_schedule="cosine", lr_warmup_steps=3, lr_min=1e-3, weight_decay=5e-2,
                log_file=str(tmp_path / f"{name}.jsonl"))
    base.update(over)
    return engine.default_config(**base)


def _records(tmp_path, name):
    return [json.loads(ln) for ln in (tmp_path / f"{name}.jsonl").read_text().splitlines()]


@pytest.mark.parametrize("grad_sync", ["powersgd", "dense", "dense-ref", "powersgd-ref"])
def test_engine_logs_lr_and_resumes_bitwise(tmp_path, monkeypatch, grad_sync):
    real_save = engine.save_checkpoint

    def save_every_epoch(path, model, sync, epoch, **kw):
        real_save(path, model, sync, epoch=epoch, **kw)
        real_save(os.path.join(os.path.dirname(path), f"epoch{epoch}.pt"), model, sync, epoch=epoch, **kw)
    monkeypatch.setattr(engine, "save_checkpoint", save_every_epoch)

    torch.manual_seed(1)
    full = engine.run_task(_cfg(tmp_path, "full", grad_sync=grad_sync, checkpoint_dir=str(tmp_path / "ck")))
    sched = LrSchedule(0.05, 4, 2, schedule="cosine", warmup_steps=3, lr_min=1e-3)
    recs = _records(tmp_path, "full")
    steps = [r for r in recs if r["kind"] == "step"]
    assert [r["step"] for r in steps] == list(range(1, 9))
    assert [r["lr"] for r in steps] == [sched.lr_at(k) for k in range(8)]  # record k + 1 = the step of index k
    assert [r["lr"] for r in recs if r["kind"] == "epoch"] == [sched.lr_at(3), sched.lr_at(7)]
    summ = recs[-1]
    assert summ["kind"] == "summary" and summ["lr_schedule"] == "cosine" and summ["weight_decay"] == 5e-2
    assert len({r["lr"] for r in steps}) == 7  # steps 2 and 3 both run at the base rate (warm-up end, cosine start)

    if grad_sync.endswith("-ref"):
        return  # the reference loops keep no checkpointable optimiser state
    torch.manual_seed(99)  # the resumed run's initialisation is replaced by the checkpoint
    res = engine.run_task(_cfg(tmp_path, "res", grad_sync=grad_sync, resume=str(tmp_path / "ck" / "epoch0.pt")))
    rsteps = [r for r in _records(tmp_path, "res") if r["kind"] == "step"]
    assert [r["step"] for r in rsteps] == [5, 6, 7, 8]
    assert [r["lr"] for r in rsteps] == [sched.lr_at(k) for k in range(4, 8)]
    for a, b in zip(full["model"].parameters(), res["model"].parameters()):
        assert torch.equal(a, b)
    assert res["param_checksum"] == full["param_checksum"]


def test_engine_defaults_log_nothing_new(tmp_path):
    torch.manual_seed(1)
    out = engine.run_task(_cfg(tmp_path, "plain", grad_sync="powersgd", lr_schedule="constant", lr_warmup_steps=0,
                               lr_min=0.0, weight_decay=0.0, training_epochs=1))
    recs = _records(tmp_path, "plain")
    assert not any("lr" in r for r in recs)
    assert "lr_schedule" not in recs[-1] and "weight_decay" not in recs[-1] and "lr_schedule" not in out


def test_weight_decay_changes_training_and_matches_torch_sgd(tmp_path):
    """dense (the CPU twin of the fused SGD kernel) against dense-ref (torch.optim.SGD with the same
    schedule through param_groups): the same model after 2 epochs, and a different one without decay."""
    outs = {}
    for name, over in (("dense", {}), ("dense-ref", {}), ("nodecay", dict(weight_decay=0.0))):
        torch.manual_seed(1)
        gs = "dense" if name == "nodecay" else name
        outs[name] = engine.run_task(_cfg(tmp_path, name, grad_sync=gs, **over))
    pa, pb, pc = ([p.detach() for p in outs[k]["model"].parameters()] for k in ("dense", "dense-ref", "nodecay"))
    for a, b in zip(pa, pb):
        assert torch.allclose(a, b, atol=1e-5, rtol=1e-4)
    assert any(not torch.allclose(a, c, atol=1e-4) for a, c in zip(pa, pc))
