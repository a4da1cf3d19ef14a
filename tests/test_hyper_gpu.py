"""The optimisers' device hyper-parameter block (csrc/hyper.h, ops/hyper.py): learning rate and
weight decay read by the update kernels at run time, so a schedule reaches a captured step.

The parameter set is the one of tests/test_dead_taps_gpu.py (local copies of its helpers): the
vector path, the scalar path with a width not divisible by 4, several P / Q chunks, one full matrix
and a 1-D parameter; ranks 4 / 8 / 16 run the wide update kernel (the rank-1 step rides in its
launch), rank 32 the MFMA update kernel plus the separate rank-1 launch."""
import numpy as np
import pytest
import torch

from network_distributed_pytorch_amd import ops
from network_distributed_pytorch_amd.ops import taps
from network_distributed_pytorch_amd.parallel.ddp import BucketedDataParallel
from network_distributed_pytorch_amd.parallel.powersgd import PowerSGDOptimizer
from network_distributed_pytorch_amd.utils.graph import StepRunner

pytestmark = pytest.mark.gpu

CENTRE, CORNER = 1 << 4, 0b110110000  # {4} and {4, 5, 7, 8}
SHAPES = [((130, 64, 3, 3), CENTRE),   # three Q row chunks, two P column chunks, n % 16 != 0
          ((18, 16, 3, 3), CORNER),
          ((32, 5, 3, 3), CENTRE),     # full width 45: the scalar (non-vector) paths
          ((32, 16, 3, 3), None),      # one full matrix
          ((50,), None)]               # a 1-D parameter
COMPACT = [True, True, True, False]
LR0, WD = 0.05, 5e-2
# rank, lazy error feedback, optimiser keywords
ARMS = [(4, True, {}), (8, True, {}), (16, True, {}), (4, False, {}), (8, False, dict(write_grad=True)),
        (4, True, dict(write_grad=True)), (4, True, dict(overlap=True, groups=2)), (32, True, {}),
        (32, True, dict(write_grad=True))]


def _f32(v):
    return float(np.float32(v))


def _dead(shape, mask):
    d = torch.zeros(shape, dtype=torch.bool)
    if mask is not None:
        for t in range(9):
            if not mask >> t & 1:
                d[:, :, t // 3, t % 3] = True
    return d


def _params(device):
    gen = torch.Generator(device="cpu").manual_seed(21)
    ps = [torch.nn.Parameter(torch.randn(s, generator=gen).to(device)) for s, _ in SHAPES]
    for p, (_, mask) in zip(ps, SHAPES):
        if mask is not None:
            taps.mark(p, 9, mask)
    return ps


def _grads(gen, device):
    out = []
    for s, mask in SHAPES:
        g = torch.randn(s, generator=gen)
        g[_dead(s, mask)] = 0.0  # exact zeros in the dead taps
        out.append(g.to(device))
    return out


@pytest.fixture(scope="module")
def grad_steps():
    """The gradients of 6 steps, drawn once and shared (never modified: every step clones them)."""
    gen = torch.Generator(device="cpu").manual_seed(5)
    dev = torch.device("cuda", 0)
    return [_grads(gen, dev) for _ in range(6)] if torch.cuda.is_available() else []


def _opt(device, on, rank, lazy=True, **kw):
    ps = _params(device)
    o = PowerSGDOptimizer(ps, lr=LR0, momentum=0.9, rank=rank, **kw)
    o.dead_taps = on
    if not lazy:
        o.lazy_ef = False
    return ps, o


def _step(ps, o, grads):
    o.zero_grad()
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    o.step()


def _same_running(oa, ob, what=""):
    """What can be compared without materialising the lazy error memory."""
    assert torch.equal(oa.x, ob.x), what
    assert torch.equal(oa.m, ob.m), what
    assert torch.equal(oa.buf.q_warm, ob.buf.q_warm), what
    assert torch.equal(oa.buf.comm_buf, ob.buf.comm_buf), what  # P-hat and the rank-1 payload


def _same(oa, ob, what=""):
    _same_running(oa, ob, what)
    assert torch.equal(oa.e, ob.e), what


# ---- 1. weight_decay = 0 through the block is the by-value step, bitwise ---------------------------
@pytest.mark.parametrize("rank,lazy,kw", ARMS)
def test_block_with_zero_decay_is_the_by_value_step(device, grad_steps, rank, lazy, kw):
    pa, oa = _opt(device, True, rank, lazy, **kw)
    pb, ob = _opt(device, True, rank, lazy, **kw)
    oa.set_hyper(LR0, 0.0)
    assert oa._hyper_on and not ob._hyper_on  # oa's kernels read the block, ob's take lr by value
    assert oa.hyper.uploads == 0              # ... which already held these values: nothing enqueued
    assert torch.equal(oa.hyper.dev.cpu(), torch.tensor([_f32(LR0), 0.0, 0.0, 0.0]))
    for step, grads in enumerate(grad_steps[:4]):
        _step(pa, oa, grads)
        _step(pb, ob, grads)
        if kw.get("write_grad"):
            for a, b in zip(pa, pb):
                assert torch.equal(a.grad, b.grad), step
        _same_running(oa, ob, step)
        oa.set_hyper(LR0, 0.0)
    _same(oa, ob)
    assert oa.hyper.uploads == 0
    assert [lay is not None for lay in oa.buf.layout] == ([False] * 4 if rank > 16 else COMPACT)
    oa.check_errors()


@pytest.mark.parametrize("n", [1, 4, 1023, 4099])
def test_sgd_momentum_block_with_zero_decay_is_bitwise(device, n):
    gen = torch.Generator(device="cpu").manual_seed(n)
    x, g, b = (torch.randn(n, generator=gen).to(device) for _ in range(3))
    x[0], g[0], b[0] = 1.0, -0.0, -0.0  # fmaf(0, 1, -0) would give +0: the wd != 0 test keeps the sign
    x2, b2 = x.clone(), b.clone()
    hyper = torch.tensor([0.1, 0.0, 0.0, 0.0], device=device)
    for _ in range(2):
        ops.sgd_momentum_(x, g, b, 0.1, 0.9, 2.0)
        ops.sgd_momentum_(x2, g, b2, 123.0, 0.9, 2.0, hyper=hyper)  # the by-value lr is ignored
    assert torch.equal(x, x2) and torch.equal(b, b2)
    assert torch.equal(torch.signbit(b), torch.signbit(b2))


# ---- 2. the lr reaches every path, the compacted one included -------------------------------------
@pytest.mark.parametrize("rank,lazy,kw", [a for a in ARMS if a[0] <= 16])
def test_lr_from_block_reaches_compact_and_full_paths(device, grad_steps, rank, lazy, kw):
    pa, oa = _opt(device, True, rank, lazy, **kw)
    pb, ob = _opt(device, False, rank, lazy, **kw)
    pc, oc = _opt(device, True, rank, lazy, **kw)  # constant lr
    for step, grads in enumerate(grad_steps[:4]):
        lr = (LR0, 0.4)[step % 2]
        for o in (oa, ob):
            o.set_hyper(lr, 0.0)
        _step(pa, oa, grads)
        _step(pb, ob, grads)
        _step(pc, oc, grads)
        if kw.get("write_grad"):
            for a, b in zip(pa, pb):
                assert torch.equal(a.grad, b.grad), step
        _same_running(oa, ob, step)
    _same(oa, ob)
    assert [lay is not None for lay in oa.buf.layout] == COMPACT
    assert all(lay is None for lay in ob.buf.layout)
    assert oa.hyper.uploads == 3  # 0.05 was there; 0.4, 0.05, 0.4 were uploaded
    for i, (a, c) in enumerate(zip(pa, pc)):  # every parameter moved differently, the compacted ones too
        assert not torch.equal(a, c), i
    oa.check_errors()


# ---- 3. weight decay against the torch twin --------------------------------------------------------
def _make_model(device):
    torch.manual_seed(3)
    m = torch.nn.Sequential(
        torch.nn.Conv2d(3, 16, 3, bias=False), torch.nn.BatchNorm2d(16), torch.nn.ReLU(),
        torch.nn.Conv2d(16, 8, 3), torch.nn.Flatten(), torch.nn.Linear(8 * 4 * 4, 10))
    return m.to(device)


@pytest.mark.parametrize("write_grad", [False, True])
def test_weight_decay_matches_torch_twin(device, write_grad):
    ma, mb, mc = _make_model(device), _make_model(device), _make_model(device)
    mb.load_state_dict(ma.state_dict())
    mc.load_state_dict(ma.state_dict())
    oa = PowerSGDOptimizer(ma.parameters(), lr=0.1, momentum=0.9, rank=4, write_grad=write_grad)
    ob = PowerSGDOptimizer(mb.parameters(), lr=0.1, momentum=0.9, rank=4, write_grad=write_grad, native=False)
    oc = PowerSGDOptimizer(mc.parameters(), lr=0.1, momentum=0.9, rank=4, write_grad=write_grad)  # no decay
    assert oa.native and not ob.native and ob.hyper is None
    torch.manual_seed(5)
    for step, lr in enumerate((0.1, 0.05, 0.2, 0.1)):
        x = torch.randn(64, 3, 8, 8, device=device)
        y = torch.randint(0, 10, (64,), device=device)
        oa.set_hyper(lr, WD)
        ob.set_hyper(lr, WD)
        for m, o in ((ma, oa), (mb, ob)):
            o.zero_grad()
            torch.nn.functional.cross_entropy(m(x), y).backward()
        if step == 0:  # the run without decay takes oa's very gradients (a library conv backward
            oc.zero_grad()  # need not repeat itself bitwise)
            for pa, pc in zip(ma.parameters(), mc.parameters()):
                pc.grad = pa.grad.clone()
            oc.step()
        oa.step()
        ob.step()
        for pa, pb in zip(ma.parameters(), mb.parameters()):
            assert torch.allclose(pa, pb, atol=1e-5, rtol=1e-4), step
        assert torch.allclose(oa.e, ob.e, atol=1e-5, rtol=1e-3), (oa.e - ob.e).abs().max()
        assert torch.allclose(oa.m, ob.m, atol=1e-5, rtol=1e-3), (oa.m - ob.m).abs().max()
        if write_grad:
            for pa, pb in zip(ma.parameters(), mb.parameters()):
                assert torch.allclose(pa.grad, pb.grad, atol=1e-5, rtol=1e-4)
        if step == 0:
            # the decay is applied after decompression: the error memory and both collectives'
            # payloads ([P-hat | rank-1], Q) are those of the run without it
            assert torch.equal(oa.e, oc.e)
            assert torch.equal(oa.buf.comm_buf, oc.buf.comm_buf) and torch.equal(oa.buf.q_memory, oc.buf.q_memory)
            assert not torch.equal(oa.x, oc.x) and not torch.equal(oa.m, oc.m)
    assert oa.bits_per_step == oc.bits_per_step and oa.collective_payloads() == oc.collective_payloads()
    oa.check_errors()


# ---- 4. weight decay keeps (and returns to) the full layout ----------------------------------------
@pytest.mark.parametrize("rank,lazy,kw", [(4, True, {}), (4, False, {}), (8, True, dict(write_grad=True))])
def test_decay_switched_on_replans_to_full(device, grad_steps, rank, lazy, kw):
    pa, oa = _opt(device, True, rank, lazy, **kw)
    pb, ob = _opt(device, False, rank, lazy, **kw)  # the full layout from the start
    for step, grads in enumerate(grad_steps[:4]):
        lr, wd = (LR0, 0.4)[step % 2], (0.0 if step < 2 else WD)
        for o in (oa, ob):
            o.set_hyper(lr, wd)
        _step(pa, oa, grads)
        _step(pb, ob, grads)
        _same_running(oa, ob, step)
        assert [lay is not None for lay in oa.buf.layout] == (COMPACT if step < 2 else [False] * 4), step
    _same(oa, ob)
    for p, (s, mask) in zip(pa, SHAPES):  # the dead taps have moved: they needed their momentum
        if mask is not None:
            d = _dead(s, mask).to(device)
            assert (oa._view(oa.m, p).view_as(p)[d] != 0).any()
    oa.check_errors()
    # with a decay from the first step nothing is ever compacted
    pc, oc = _opt(device, True, rank, lazy, weight_decay=WD, **kw)
    _step(pc, oc, grad_steps[0])
    assert all(lay is None for lay in oc.buf.layout)
    oc.check_errors()


# ---- 5. the dense arm -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4, 1023, 4099])
def test_sgd_momentum_weight_decay_matches_fp64(device, n):
    gen = torch.Generator(device="cpu").manual_seed(100 + n)
    x, g, b = (torch.randn(n, generator=gen).to(device) for _ in range(3))
    lr, wd, mu, div = _f32(0.1), _f32(1e-2), _f32(0.9), 2.0
    hyper = torch.tensor([lr, wd, 0.0, 0.0], device=device)
    x64, g64, b64 = x.double(), g.double(), b.double()
    ops.sgd_momentum_(x, g, b, 7.0, 0.9, div, hyper=hyper)
    d = g64 / div + wd * x64
    b64 = mu * b64 + d
    x64 = x64 - lr * b64
    assert torch.allclose(b.double(), b64, atol=1e-6, rtol=0) and torch.allclose(x.double(), x64, atol=1e-6, rtol=0)
    with pytest.raises(ValueError, match="hyper"):
        ops.sgd_momentum_(x, g, b, 0.1, 0.9, div, weight_decay=1e-2)  # no by-value decay on the device


def test_bucketed_data_parallel_follows_torch_sgd(device):
    torch.manual_seed(2)
    ma = torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.Tanh(), torch.nn.Linear(19, 5)).to(device)
    mb = torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.Tanh(), torch.nn.Linear(19, 5)).to(device)
    mb.load_state_dict(ma.state_dict())
    ddp = BucketedDataParallel(ma, lr=0.1, momentum=0.9)
    ref = torch.optim.SGD(mb.parameters(), lr=0.1, momentum=0.9)
    for lr in (0.1, 0.4, 0.05):
        x = torch.randn(16, 37, device=device)
        ddp.set_hyper(lr, 1e-2)
        for group in ref.param_groups:
            group["lr"], group["weight_decay"] = lr, 1e-2
        ddp.zero_grad()
        ref.zero_grad()
        ma(x).square().mean().backward()
        mb(x).square().mean().backward()
        ddp.step()
        ref.step()
    for a, b in zip(ma.parameters(), mb.parameters()):
        assert torch.allclose(a, b, atol=1e-5, rtol=1e-4)
    sd = ddp.state_dict()
    assert sd["weight_decay"] == _f32(1e-2) and sd["lr"] == _f32(0.05)
    del sd["weight_decay"]
    ddp.load_state_dict(sd)
    torch.cuda.synchronize()
    assert ddp.weight_decay == 0.0 and torch.equal(ddp.hyper.dev.cpu(), torch.tensor([_f32(0.05), 0.0, 0.0, 0.0]))


# ---- 6. a captured step follows the block ---------------------------------------------------------
@pytest.mark.parametrize("rank,kw", [(4, {}), (4, dict(overlap=True, groups=2)), (8, dict(write_grad=True)),
                                     (32, {})])
def test_replay_follows_the_block(device, grad_steps, rank, kw):
    """6 replays with lr alternating 0.05 / 0.4 (8x apart) and a decay, against the eager loop: an
    upload that lands one step early or late cannot pass.  With overlap groups the step is two graphs
    (compute + comm) and nothing joins the streams between the replays."""
    lrs = [(LR0, 0.4)[k % 2] for k in range(6)]
    pe, oe = _opt(device, True, rank, **kw)
    for lr, grads in zip(lrs, grad_steps):
        oe.set_hyper(lr, WD)
        _step(pe, oe, grads)

    pg, og = _opt(device, True, rank, **kw)
    static = [g.clone() for g in grad_steps[0]]

    def pre():
        og.zero_grad()
        for p, s in zip(pg, static):
            p.grad = s.clone()  # inside the graph: the step never reads (or, write_grad, writes) `static`
    runner = StepRunner(pre, og, mode="full", warmup=2)
    for lr, grads in zip(lrs, grad_steps):
        for s, g in zip(static, grads):
            s.copy_(g)
        og.set_hyper(lr, WD)
        runner()
    runner.join()
    torch.cuda.synchronize()
    assert runner.replays == 6 and bool(runner.side_graphs) == bool(kw.get("overlap"))
    assert og.hyper.uploads == 6 and og.step_count == 6
    _same(og, oe)
    if kw.get("write_grad"):
        for a, b in zip(pg, pe):
            assert torch.equal(a.grad, b.grad)
    og.check_errors()
    with pytest.raises(RuntimeError, match="weight_decay"):
        og.set_hyper(LR0, 0.0)  # the captured step froze the full plan


def test_by_value_capture_refuses_a_schedule(device, grad_steps):
    pg, og = _opt(device, True, 4)
    static = [g.clone() for g in grad_steps[0]]

    def pre():
        og.zero_grad()
        for p, s in zip(pg, static):
            p.grad = s.clone()
    runner = StepRunner(pre, og, mode="full", warmup=1)
    runner()
    og.set_hyper(LR0, 0.0)  # unchanged values are fine
    with pytest.raises(RuntimeError, match="by value"):
        og.set_hyper(0.4, 0.0)
    torch.cuda.synchronize()


# ---- 7. checkpoint ----------------------------------------------------------------------------------
@pytest.mark.parametrize("rank", [4, 32])
def test_checkpoint_carries_decay_and_reuploads(device, grad_steps, rank):
    lrs = [LR0, 0.4, 0.4, LR0]
    pr, ref = _opt(device, True, rank)
    for lr, grads in zip(lrs, grad_steps):
        ref.set_hyper(lr, WD)
        _step(pr, ref, grads)
    pa, oa = _opt(device, True, rank)
    for lr, grads in zip(lrs[:2], grad_steps):
        oa.set_hyper(lr, WD)
        _step(pa, oa, grads)
    sd = oa.state_dict()
    assert sd["weight_decay"] == _f32(WD) and sd["lr"] == _f32(0.4)
    pb, ob = _opt(device, True, rank)
    with torch.no_grad():
        for a, b in zip(pa, pb):
            b.copy_(a)
    ob.load_state_dict(sd)
    torch.cuda.synchronize()
    assert torch.equal(ob.hyper.dev.cpu(), torch.tensor([_f32(0.4), _f32(WD), 0.0, 0.0]))
    _step(pb, ob, grad_steps[2])  # lr 0.4 and the decay come from the checkpoint
    ob.set_hyper(lrs[3], WD)
    _step(pb, ob, grad_steps[3])
    _same(ob, ref)
    old = dict(sd)
    del old["weight_decay"]  # a checkpoint from before the key existed
    ob.load_state_dict(old)
    torch.cuda.synchronize()
    assert ob.weight_decay == 0.0 and ob.hyper.dev[1].item() == 0.0


# ---- 8. the engine: a schedule reaches the captured step, the ragged eager step included -------------
@pytest.mark.parametrize("grad_sync", ["powersgd", "dense"])
def test_engine_schedule_in_graph_mode(device, tmp_path, grad_sync):
    import json

    from network_distributed_pytorch_amd import engine
    from network_distributed_pytorch_amd.utils.schedule import LrSchedule

    def run(mode, **over):
        torch.manual_seed(0)  # the engine builds the model from the current RNG
        name = f"{mode}{len(over)}"
        cfg = engine.default_config(**dict(dict(
            task="mlp", grad_sync=grad_sync, training_epochs=2, dataset_size=200, global_batch=64, graph_mode=mode,
            verbose=False, learning_rate=0.05, lr_schedule="cosine", lr_warmup_steps=2, lr_min=1e-3, weight_decay=5e-2,
            log_file=str(tmp_path / f"{name}.jsonl")), **over))
        out = engine.run_task(cfg)
        recs = [json.loads(ln) for ln in (tmp_path / f"{name}.jsonl").read_text().splitlines()]
        return out, [r["lr"] for r in recs if r["kind"] == "step"]

    out_g, lr_g = run("full")
    out_e, lr_e = run("none")
    out_c, _ = run("full", lr_schedule="constant", lr_warmup_steps=0, lr_min=0.0)  # decay only
    sched = LrSchedule(0.05, 4, 2, schedule="cosine", warmup_steps=2, lr_min=1e-3)
    assert out_g["graph_mode"] == "full" and out_g["steps"] == 8  # 64 + 64 + 64 + 8 per epoch: one ragged step
    assert lr_g == lr_e == [sched.lr_at(k) for k in range(8)]
    # graph and eager run the same kernels on the same values: the existing graph-against-eager bound
    tol = 1e-6 * abs(out_e["param_checksum"]) + 1e-3
    assert abs(out_g["param_checksum"] - out_e["param_checksum"]) <= tol
    assert abs(out_g["epoch_losses"][1] - out_e["epoch_losses"][1]) <= 1e-4 * abs(out_e["epoch_losses"][1])
    # ... and the schedule did reach the replays: the constant-lr run ends somewhere else
    assert abs(out_c["param_checksum"] - out_e["param_checksum"]) > 10 * tol
    opt = getattr(out_g["sync"], "opt", None) or out_g["sync"].ddp
    assert opt.hyper.uploads == 7  # steps 1 and 2 share the base rate (warm-up end, cosine start)
