"""``grad_sync="powersgd-adamw"`` without a GPU: the torch twin of the fused engine's AdamW arm
(parallel/powersgd.py ``_step_torch``) against the test-only rule of tests/adamw_rule.py, the error
memory and the wire against the SGD engine, the ``GradSync`` contract, configuration, checkpoints, the
engine on the CPU MLP task and two gloo ranks."""
import json
import os

import numpy as np
import pytest
import torch

from network_distributed_pytorch_amd import engine
from network_distributed_pytorch_amd.parallel.comm import Communicator
from network_distributed_pytorch_amd.parallel.powersgd import PowerSGDOptimizer
from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync
from network_distributed_pytorch_amd.utils.config import ConfigError, validate_config
from network_distributed_pytorch_amd.utils.launcher import spawn
from tests import adamw_rule as rule
from tests import psgd_adam_helpers as H

_bits = H.bits


def _opt(model, **kw):
    args = dict(lr=H.HYPER[0][0], rank=H.RANK, native=False, optimizer="adamw", betas=H.BETAS, eps_adam=H.EPS)
    args.update(kw)
    return PowerSGDOptimizer(model.parameters(), **args)


# ---- 1. the twin against the rule ---------------------------------------------------------------------
@pytest.mark.parametrize("decay_1d", [True, False])
def test_twin_equals_the_rule_on_the_decompressed_gradient(decay_1d):
    model = H.make_model()
    opt = _opt(model, write_grad=True, decay_1d=decay_1d)
    assert opt.buf.ranks == [4, 3] and [p.numel() for p in opt.rank1] == [5, 3]
    assert opt.adam_stats() == {"b1pow": 1.0, "b2pow": 1.0, "steps": 0}
    moved = 0
    for k, (lr, wd) in enumerate(H.HYPER):
        opt.set_hyper(lr, wd)
        pre = [(p.detach().clone(), opt._view(opt._m, p).clone(), opt._view(opt._v, p).clone()) for p in opt.params]
        st = opt.adam_stats()
        block = (np.float32(st["b1pow"]), np.float32(st["b2pow"]), st["steps"])
        H.backward(opt, model, k)
        raw = [p.grad.clone() for p in opt.params]
        opt.step()
        want_block = None
        for p, (x0, m0, v0), g_raw in zip(opt.params, pre, raw):
            o = p.grad  # write_grad: the decompressed (matrices) / averaged (<=1-D) gradient
            if p.dim() <= 1:
                assert np.array_equal(_bits(o), _bits(g_raw))  # one process: rank1 / 1
            else:
                assert not torch.equal(o, g_raw)  # rank 4 of a 5 x 7 matrix: compressed
            x1, m1, v1, want_block = rule.step(x0.numpy(), o.numpy(), m0.numpy(), v0.numpy(), block, opt.lr,
                                               opt.weight_decay, *H.BETAS, H.EPS, 1.0, decay_1d or p.dim() > 1)
            assert rule.same_bits(x1, p.detach().numpy().ravel()), (k, tuple(p.shape))
            assert rule.same_bits(m1, opt._view(opt._m, p).numpy()) and rule.same_bits(v1, opt._view(opt._v, p).numpy())
            moved += int(not torch.equal(x0, p.detach()))
        st = opt.adam_stats()
        assert (np.float32(st["b1pow"]), np.float32(st["b2pow"]), st["steps"]) == want_block and st["steps"] == k + 1
    assert moved == 3 * len(opt.params)


def test_decay_1d_false_leaves_the_biases_undecayed():
    outs = []
    for decay_1d in (True, False):
        model = H.make_model()
        opt = _opt(model, decay_1d=decay_1d, weight_decay=0.5)
        H.backward(opt, model, 0)
        opt.step()
        outs.append([p.detach().clone() for p in opt.params])
    for a, b in zip(*outs):
        assert torch.equal(a, b) == (a.dim() > 1)


# ---- 2. error memory and wire -------------------------------------------------------------------------
def test_error_memory_queries_and_bits_are_the_sgd_engines():
    res = []
    for kw in (dict(optimizer="sgd"), dict(optimizer="adamw", weight_decay=0.1)):
        model = H.make_model()
        opt = _opt(model, **kw)
        H.backward(opt, model, 0)
        res.append((opt.step(), opt.e.clone(), opt.buf.q_warm.clone(), opt.bits_per_step, opt.x.clone()))
    (bs, es, qs, ps, xs), (ba, ea, qa, pa, xa) = res
    assert ba == bs and pa == ps
    assert np.array_equal(_bits(ea), _bits(es)) and np.array_equal(_bits(qa), _bits(qs))
    assert float(ea.abs().max()) > 0 and not torch.equal(xa, xs)  # another update rule on the same wire


# ---- 3. the GradSync contract -------------------------------------------------------------------------
def test_the_new_kind_answers_the_whole_gradsync_contract():
    from network_distributed_pytorch_amd.parallel.sync import GradSync
    from tests.test_gradsync_cpu import _mlp, _step

    model = _mlp()
    sync = build_grad_sync("powersgd-adamw", model, Communicator(), lr=0.05, momentum=0.9, rank=2)
    assert isinstance(sync, GradSync) and sync.optimizer == "adamw"
    assert sync.plan_hyper([(0.05, 0.0), (0.04, 0.0)]) is None
    sync.set_hyper(0.05, 0.0)
    sync.prepare()
    assert sync.adam_stats()["steps"] == 0
    assert _step(sync, model, 0) == 8 * sync.bytes_per_step
    assert sync.adam_stats()["steps"] == 1
    sync.count_step()
    sync.check_errors()
    assert sync.clip_stats() is None
    sync.attach_ema(None)
    snap = sync.snapshot()
    _step(sync, model, 1)
    assert sync.adam_stats()["steps"] == 2
    sync.restore(snap)
    assert sync.adam_stats()["steps"] == 1
    payloads = sync.collective_payloads()
    assert isinstance(payloads, list) and sync.collectives_per_step == 0
    sd = sync.state_dict()
    sync.load_state_dict(sd)
    phases = sync.phases()
    arena = sync.flat_weights
    assert arena is sync.x and arena.dim() == 1 and sync.opt is sync
    assert all(p.data_ptr() >= arena.data_ptr() and
               p.data_ptr() + 4 * p.numel() <= arena.data_ptr() + 4 * arena.numel() for p in model.parameters())
    assert isinstance(snap, dict) and phases and all(callable(fn) for fn, _ in phases)
    assert sum(payloads) >= sync.bytes_per_step > 0
    for fn, _ in phases:  # the piecewise step advances the block once, too
        fn()
    assert sync.adam_stats()["steps"] == 2
    # with SGD the engine has nothing to say about Adam and keeps no second moment
    sgd = build_grad_sync("powersgd", _mlp(), Communicator(), lr=0.05, rank=2)
    assert sgd.adam_stats() is None and not hasattr(sgd, "_v") and "optimizer" not in sgd.state_dict()


# ---- 4. configuration, constructor, state -------------------------------------------------------------
def test_config_keys_normalise_and_refuse():
    for given in ({}, {"optimizer": "sgd"}, {"optimizer": "adamw"}):
        c = validate_config({"grad_sync": "powersgd-adamw", **given})
        assert c["optimizer"] == "adamw"
    with pytest.raises(ConfigError, match="reuse_query"):
        validate_config({"grad_sync": "powersgd-adamw", "graph_mode": "full", "reuse_query": False})
    with pytest.raises(ConfigError, match="powersgd-adamw.*max_grad_norm"):
        validate_config({"grad_sync": "powersgd-adamw", "overlap": True, "max_grad_norm": 1.0})
    with pytest.raises(ConfigError, match="adamw"):  # "powersgd" itself stays SGD-only
        validate_config({"grad_sync": "powersgd", "optimizer": "adamw"})
    with pytest.raises(ConfigError, match="optimizer"):
        validate_config({"grad_sync": "powersgd-adamw", "optimizer": "nadam"})
    assert validate_config({"grad_sync": "powersgd"})["optimizer"] == "sgd"


def test_build_grad_sync_and_constructor_refusals():
    comm = Communicator()
    with pytest.raises(ValueError, match="no AdamW"):
        build_grad_sync("powersgd", H.make_model(), comm, optimizer="adamw")
    with pytest.raises(ValueError, match="unknown optimizer"):
        build_grad_sync("powersgd-adamw", H.make_model(), comm, optimizer="nadam")
    with pytest.raises(ValueError, match="beta1"):
        build_grad_sync("powersgd-adamw", H.make_model(), comm, betas=(1.0, 0.9))
    with pytest.raises(ValueError, match="unknown optimizer"):
        PowerSGDOptimizer(H.make_model().parameters(), lr=0.1, native=False, optimizer="nadam")
    s = build_grad_sync("powersgd-adamw", H.make_model(), comm, lr=0.01, rank=2, betas=(0.8, 0.9), eps=1e-6,
                        decay_1d=False, write_grad=True, reuse_query=True, overlap=None, groups=None)
    assert (s.beta1, s.beta2, s.eps_adam, s.decay_1d, s.write_grad) == (0.8, 0.9, 1e-6, False, True)
    assert s.eps == 1e-8  # the orthogonaliser's eps is another argument
    big = torch.nn.Linear(20, 18)
    with pytest.raises(ValueError, match="rank 17"):
        PowerSGDOptimizer(big.parameters(), lr=0.1, rank=17, native=False, optimizer="adamw")
    PowerSGDOptimizer(big.parameters(), lr=0.1, rank=17, native=False)  # SGD keeps the narrow plans
    PowerSGDOptimizer(torch.nn.Linear(20, 18).parameters(), lr=0.1, rank=16, native=False, optimizer="adamw")
    # the full layout always: whatever the decay
    assert s._wanted_supports() == [(0, 0)] * len(s.high)
    s.set_hyper(0.01, 0.3)
    s.set_hyper(0.01, 0.0)  # toggling the decay is never refused: the plan does not depend on it


def _steps(opt, model, ks):
    for k in ks:
        opt.set_hyper(*H.HYPER[k % 3])
        H.backward(opt, model, k)
        opt.step()


def test_snapshot_state_dict_round_trips_and_optimizer_mismatch():
    ma, mb, ms = H.make_model(), H.make_model(), H.make_model()
    a, b, s = _opt(ma), _opt(mb), _opt(ms, optimizer="sgd")
    _steps(a, ma, range(2))
    _steps(s, ms, range(2))
    snap = a.snapshot()
    at_snap = H.state_bits(a)
    sd = a.state_dict()
    assert sd["optimizer"] == "adamw" and sd["steps"] == 2 and torch.equal(sd["exp_avg_sq"], a._v)
    assert "optimizer" not in s.state_dict() and "exp_avg_sq" not in s.state_dict()
    _steps(a, ma, range(2, 4))
    first = H.state_bits(a)
    assert first["block"]["steps"] == 4 and not np.array_equal(first["v"], at_snap["v"])
    a.restore(snap)
    H.same_state(H.state_bits(a), at_snap)
    _steps(a, ma, range(2, 4))
    H.same_state(H.state_bits(a), first)
    # a fresh optimiser continues bitwise from the state dict (weights travel with the model)
    b.x.copy_(torch.zeros_like(b.x))
    b.load_state_dict(sd)
    b.x.copy_(torch.from_numpy(at_snap["x"]).view(torch.float32))
    H.same_state(H.state_bits(b), at_snap)
    _steps(b, mb, range(2, 4))
    H.same_state(H.state_bits(b), first)
    with pytest.raises(ValueError, match="sgd optimizer state"):
        a.load_state_dict(s.state_dict())
    with pytest.raises(ValueError, match="adamw optimizer state"):
        s.load_state_dict(sd)


def _run(tmp_path, name, grad_sync="powersgd-adamw", epochs=2, **kw):
    cfg = engine.default_config(task="mlp", grad_sync=grad_sync, dataset_size=256, global_batch=32,
                                training_epochs=epochs, verbose=False, learning_rate=0.01, reducer_rank=2,
                                log_file=str(tmp_path / f"{name}.jsonl"), **kw)
    torch.manual_seed(1)
    out = engine.run_task(cfg)
    recs = [json.loads(ln) for ln in (tmp_path / f"{name}.jsonl").read_text().splitlines()]
    return out, recs


ADAM = dict(lr_schedule="cosine", lr_warmup_steps=2, weight_decay=0.05, decay_1d=False)


def test_engine_records_and_resume_bitwise(tmp_path, monkeypatch):
    real_save = engine.save_checkpoint

    def save_every_epoch(path, model, sync, epoch, **kw):  # the mid-run checkpoint survives the later epochs
        real_save(path, model, sync, epoch=epoch, **kw)
        real_save(os.path.join(os.path.dirname(path), f"epoch{epoch}.pt"), model, sync, epoch=epoch, **kw)
    monkeypatch.setattr(engine, "save_checkpoint", save_every_epoch)
    ck = tmp_path / "ck"
    full, recs = _run(tmp_path, "full", checkpoint_dir=str(ck), **ADAM)
    assert full["steps"] == 16 and full["optimizer"] == "adamw" and full["adam_steps"] == 16
    assert [r["adam_steps"] for r in recs if r["kind"] == "epoch"] == [8, 16]
    assert np.isfinite(full["epoch_losses"]).all() and full["epoch_losses"][1] < full["epoch_losses"][0]
    state = torch.load(ck / "epoch0.pt", map_location="cpu", weights_only=True)
    assert state["sync"]["optimizer"] == "adamw" and state["sync"]["steps"] == 8
    torch.manual_seed(99)
    res, _ = _run(tmp_path, "resumed", resume=str(ck / "epoch0.pt"), **ADAM)
    assert res["adam_steps"] == 16
    H.same_state(H.state_bits(res["sync"]), H.state_bits(full["sync"]))  # moments and the block included
    for a, b in zip(full["model"].parameters(), res["model"].parameters()):
        assert np.array_equal(_bits(a), _bits(b))
    # an SGD checkpoint of the same engine into the AdamW kind says what is wrong
    ck2 = tmp_path / "ck2"
    sgd, recs_sgd = _run(tmp_path, "plain", "powersgd", epochs=1, checkpoint_dir=str(ck2))
    assert not any("optimizer" in r or "adam_steps" in r for r in recs_sgd) and "optimizer" not in sgd
    with pytest.raises(ValueError, match="sgd optimizer state"):
        _run(tmp_path, "bad", resume=str(ck2 / "epoch0.pt"), **ADAM)


# ---- 5. two gloo ranks --------------------------------------------------------------------------------
@pytest.mark.parametrize("decay_1d,same_mats", [(True, False), (False, True)])
def test_two_ranks_agree_and_equal_the_twin_on_averaged_inputs(tmp_path, decay_1d, same_mats):
    """Replicas end identical whatever each rank's gradients.  Against one process the comparison is
    bitwise where averaging commutes with the arithmetic: the <=1-D group (sum of two, halved) always,
    the matrices when both ranks hold the same gradient (P + P and its half are exact; the product of an
    averaged matrix is not the average of the products bit for bit)."""
    steps = 3
    spawn(H.psgd_adam_rank_body, 2, args=(str(tmp_path), steps, decay_1d, same_mats))
    a, b = (torch.load(os.path.join(tmp_path, f"psgd_adam_rank{r}.pt"), weights_only=True) for r in range(2))
    assert a["block"] == b["block"] and a["block"]["steps"] == steps
    for k in ("init", "x", "m", "v", "q"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k  # broadcast from rank 0, then identical replicas
    assert any(not torch.equal(g, h) for g, h in zip(a["grads"][0], b["grads"][0]))
    assert torch.isfinite(a["x"]).all() and not torch.equal(a["x"], a["init"])
    if not same_mats:
        assert not torch.equal(a["e"], b["e"])  # the error memory is each rank's own
        return
    model = H.make_model()
    one = _opt(model, decay_1d=decay_1d)
    one.x.copy_(a["init"])
    for k in range(steps):
        one.set_hyper(*H.HYPER[k % 3])
        one.zero_grad()
        for p, g, h in zip(model.parameters(), a["grads"][k], b["grads"][k]):
            p.grad = (g + h) / 2  # N = 2 divides exactly
        one.step()
    for k, t in (("x", one.x), ("m", one.m), ("v", one._v), ("e", one.e), ("q", one.buf.q_warm)):
        assert np.array_equal(_bits(t), _bits(a[k])), k
    assert one.adam_stats() == a["block"]
