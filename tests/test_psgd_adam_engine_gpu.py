"""``grad_sync="powersgd-adamw"`` on the device: the engine's AdamW launches against the CPU rule on the
device's own decompressed gradient, the captured step against the eager one, overlap groups against the
serial step (the block advancing once per step whichever launch is the last), the engine on a small
DistilBERT, and the snapshot with everything attached."""
import os

import numpy as np
import pytest
import torch

from network_distributed_pytorch_amd import engine, ops
from network_distributed_pytorch_amd.parallel.comm import Communicator
from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync
from network_distributed_pytorch_amd.utils.graph import StepRunner
from network_distributed_pytorch_amd.utils.schedule import LrSchedule
from tests import adamw_rule as rule
from tests import psgd_adam_helpers as H

pytestmark = pytest.mark.gpu

F = np.float32


def _sync(model, device, **kw):
    args = dict(lr=H.HYPER[0][0], rank=H.RANK, betas=H.BETAS, eps=H.EPS)
    args.update(kw)
    return build_grad_sync("powersgd-adamw", model, Communicator(device=device), **args)


def _state(s):
    torch.cuda.synchronize()
    return {"x": s.x.clone(), "m": s.m.clone(), "v": s._v.clone(), "e": s.e.clone(), "q": s.buf.q_warm.clone()}


def _same(a, b, what=""):
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{what}: {k}"


# ---- 1. the device engine against the rule on its own o -----------------------------------------------
@pytest.mark.parametrize("decay_1d", [True, False])
def test_device_step_is_the_rule_on_the_devices_decompressed_gradient(device, decay_1d):
    model = H.make_model().to(device)
    s = _sync(model, device, write_grad=True, decay_1d=decay_1d)
    assert s.native and s.lazy_ef and s.adam_stats() == {"b1pow": 1.0, "b2pow": 1.0, "steps": 0}
    for k, (lr, wd) in enumerate(H.HYPER):
        s.set_hyper(lr, wd)
        pre = [(p.detach().cpu().clone(), s._view(s._m, p).cpu().clone(), s._view(s._v, p).cpu().clone()) for p in s.params]
        st = s.adam_stats()
        block = (F(st["b1pow"]), F(st["b2pow"]), st["steps"])
        H.backward(s, model, k, device=device)
        s.step()
        torch.cuda.synchronize()
        want_block = None
        for p, (x0, m0, v0) in zip(s.params, pre):
            o = p.grad.cpu()
            x1, m1, v1, want_block = rule.step_arrays(x0.numpy(), o.numpy(), m0.numpy(), v0.numpy(), block, s.lr,
                                                      s.weight_decay, *H.BETAS, H.EPS, 1.0, decay_1d or p.dim() > 1)
            assert rule.same_bits(x1, p.detach().cpu().numpy().ravel()), (k, tuple(p.shape))
            assert rule.same_bits(m1, s._view(s._m, p).cpu().numpy()), (k, tuple(p.shape))
            assert rule.same_bits(v1, s._view(s._v, p).cpu().numpy()), (k, tuple(p.shape))
        st = s.adam_stats()
        assert (F(st["b1pow"]), F(st["b2pow"]), st["steps"]) == want_block and st["steps"] == k + 1
    assert not s._adam_ctr.any()
    s.check_errors()


# ---- 2. / 3. captured, piecewise and overlapped steps against the serial eager one ---------------------
def _net(device, bias):
    torch.manual_seed(11)
    dims = (40, 64, 48, 33, 20, 10)
    layers = []
    for a, b in zip(dims, dims[1:]):
        layers += [torch.nn.Linear(a, b, bias=bias), torch.nn.Tanh()]
    return torch.nn.Sequential(*layers[:-1]).to(device)


def _hyper(k, steps):
    return LrSchedule(0.02, steps, 1, schedule="cosine", warmup_steps=2, lr_min=1e-4).lr_at(k), 0.05


def _train(device, mode, steps, bias=True, **kw):
    model = _net(device, bias)
    s = _sync(model, device, lr=0.02, decay_1d=False, **kw)
    g = torch.Generator().manual_seed(2)
    batches = [(torch.randn(16, 40, generator=g).to(device), torch.randint(0, 10, (16,), generator=g).to(device))
               for _ in range(steps)]
    static = [batches[0][0].clone(), batches[0][1].clone()]

    def pre():
        s.zero_grad()
        torch.nn.functional.cross_entropy(model(static[0]), static[1]).backward()
    runner = StepRunner(pre, s, mode=mode, warmup=2)
    for k, (x, y) in enumerate(batches):
        static[0].copy_(x)
        static[1].copy_(y)
        s.set_hyper(*_hyper(k, steps))
        runner()
        if k == 0:
            runner.join()
            torch.cuda.synchronize()
            assert s.adam_stats()["steps"] == 1  # the warm-up steps left no trace: this was step 1
    runner.join()
    torch.cuda.synchronize()
    s.check_errors()
    assert not s._adam_ctr.any()
    return _state(s), s.adam_stats(), runner


@pytest.mark.parametrize("mode", ["full", "piecewise"])
def test_captured_step_equals_eager(device, mode):
    steps = 6
    eager, blk_e, _ = _train(device, "none", steps)
    graph, blk_g, runner = _train(device, mode, steps)
    assert runner.replays == steps
    assert blk_g == blk_e and blk_g["steps"] == steps
    _same(graph, eager, mode)
    assert float(graph["v"].abs().max()) > 0 and float(graph["e"].abs().max()) > 0


@pytest.mark.parametrize("bias", [True, False], ids=["with-1d", "no-1d"])
@pytest.mark.parametrize("groups", [2, 4])
@pytest.mark.parametrize("mode", ["none", "full"])
def test_overlap_groups_equal_the_serial_step(device, mode, groups, bias):
    """with a <=1-D group the rank-1 launch advances the block, without one the last group's launch does"""
    steps = 3
    serial, blk_s, _ = _train(device, "none", steps, bias=bias, overlap=False)
    over, blk_o, runner = _train(device, mode, steps, bias=bias, overlap=True, groups=groups)
    assert blk_o == blk_s and blk_o["steps"] == steps  # once per step, whichever launch came last
    _same(over, serial, f"{mode} {groups} groups")
    if mode == "full":
        assert runner.side_graphs


# ---- 4. the engine ------------------------------------------------------------------------------------
def test_engine_distilbert_graph_equals_eager_and_resumes_bitwise(device, monkeypatch, tmp_path):
    from network_distributed_pytorch_amd.models import distilbert_base

    real = engine.build_model

    def small(name, num_classes):
        if name != "distilbert":
            return real(name, num_classes)
        return distilbert_base(n_layers=2, dropout=0.0, attention_dropout=0.0, seq_classif_dropout=0.0)
    monkeypatch.setattr(engine, "build_model", small)
    real_save = engine.save_checkpoint

    def keep_epoch0(path, model, sync, epoch, **kw):  # the mid-run checkpoint survives the later epoch
        real_save(path if epoch else os.path.join(os.path.dirname(path), "epoch0.pt"), model, sync, epoch=epoch, **kw)
    monkeypatch.setattr(engine, "save_checkpoint", keep_epoch0)

    def run(mode, **kw):
        cfg = engine.default_config(task="imdb", grad_sync="powersgd-adamw", decay_1d=False, seq_len=64, dataset_size=16,
                                    global_batch=8, training_epochs=2, learning_rate=5e-5, weight_decay=0.01,
                                    lr_schedule="cosine", graph_mode=mode, verbose=False, reducer_rank=4, **kw)
        torch.manual_seed(3)
        return engine.run_task(cfg)
    eager = run("none")
    graph = run("auto", checkpoint_dir=str(tmp_path))
    assert eager["graph_mode"] == "none" and graph["graph_mode"] != "none"
    assert graph["optimizer"] == "adamw" and graph["adam_steps"] == eager["adam_steps"] == graph["steps"] == 4
    _same(_state(graph["sync"]), _state(eager["sync"]), "graph against eager")
    assert graph["epoch_losses"] == eager["epoch_losses"]
    resumed = run("auto", resume=str(tmp_path / "epoch0.pt"))
    assert resumed["adam_steps"] == 4 and resumed["sync"].adam_stats() == graph["sync"].adam_stats()
    _same(_state(resumed["sync"]), _state(graph["sync"]), "resumed against uninterrupted")


# ---- 5. EMA + clip + AdamW: the snapshot ---------------------------------------------------------------
def test_snapshot_round_trip_with_ema_and_clip(device):
    model = H.make_model().to(device)
    s = _sync(model, device, max_grad_norm=0.05, decay_1d=False)
    ema = ops.WeightEma([p.detach() for p in model.parameters()], 0.9)
    s.attach_ema(ema)

    def steps(ks):
        for k in ks:
            s.set_hyper(*H.HYPER[k % 3])
            H.backward(s, model, k, device=device)
            s.step()

    def full_state():
        st = _state(s)
        st["ema"] = ema.arena.clone()
        return st, s.adam_stats(), s.clip_stats(), ema.read()
    steps(range(2))
    snap = s.snapshot()
    at_snap = full_state()
    steps(range(2, 4))
    first = full_state()
    assert first[1]["steps"] == 4 and first[2]["steps"] == 4 and first[2]["clipped"] > 0 and first[3]["updates"] == 4
    assert not torch.equal(first[0]["v"], at_snap[0]["v"])
    s.restore(snap)
    back = full_state()
    _same(back[0], at_snap[0], "restored")
    assert back[1:] == at_snap[1:]
    steps(range(2, 4))
    again = full_state()
    _same(again[0], first[0], "continued")
    assert again[1:] == first[1:]
