"""Global-norm gradient clipping on the device (csrc/gradclip.hip, ops/gradclip.py): the norm
kernel against an fp64 reference, the scale kernel bitwise, non-finite inputs against
``torch.nn.utils.clip_grad_norm_``, determinism, hipGraph replay, both optimisers and the engine.

The PowerSGD parameter set is the one of tests/test_hyper_gpu.py (local copies of its helpers)."""
import json
import math

import numpy as np
import pytest
import torch

from network_distributed_pytorch_amd import engine, ops
from network_distributed_pytorch_amd.ops import taps
from network_distributed_pytorch_amd.ops.gradclip import GradClip
from network_distributed_pytorch_amd.parallel.ddp import BucketedDataParallel
from network_distributed_pytorch_amd.parallel.powersgd import PowerSGDOptimizer
from network_distributed_pytorch_amd.utils.graph import StepRunner

from .ema_cases import BIG

pytestmark = pytest.mark.gpu

INF = float("inf")
GUARD = 1234.5
SINGLES = [1, 3, 4, 5, 255, 256, 257, 2047, 2048, 2049, 3 * 2048 + 7]
# name -> (slice lengths, element offset of the first slice in the aligned buffer, value span)
CASES = {f"n{n}": ([n], 0, False) for n in SINGLES}
CASES.update({
    "mix": (SINGLES, 0, False),
    "mix_reversed": (SINGLES[::-1], 0, False),
    "offset_by_one": ([2049, 5, 2 * 2048 + 3], 1, False),  # no slice 16-byte aligned: the scalar path
    "zero_length": ([5, 0, 300], 0, False),
    "value_span": ([4, 300, 2049], 0, True),
})


def _ulp(x: float) -> float:
    return float(np.spacing(np.float32(abs(x))))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _layout(lengths, first):
    """Slices of one flat buffer with >= 4 guard elements around each; with first == 0 every slice
    starts 16-byte aligned (the float4 path), with first == 1 none does."""
    spans, o = [], 4 + first
    for n in lengths:
        spans.append((o, n))
        o = (o + n + 3) // 4 * 4 + 4 + first
    return spans, o + 4


def _make(name, device, seed=0):
    lengths, first, span = CASES[name]
    spans, total = _layout(lengths, first)
    gen = torch.Generator().manual_seed(seed)
    buf = torch.full((total,), GUARD)
    mask = torch.ones(total, dtype=torch.bool)  # True: a guard element
    for i, (o, n) in enumerate(spans):
        v = torch.randn(n, generator=gen)
        if span:  # magnitudes from 1e-20 to 1e25 across the list
            v = v * (1e-20, 1.0, 1e25)[i % 3]
        buf[o: o + n] = v
        mask[o: o + n] = False
    buf = buf.to(device)
    views = [buf[o: o + n] for o, n in spans]
    if first == 0:
        assert all(v.data_ptr() % 16 == 0 for v in views)
    else:
        assert all(v.data_ptr() % 16 != 0 for v in views if v.numel())
    return buf, views, mask.to(device)


def _ref_norm(views, div):
    s = sum(float(v.double().pow(2).sum()) for v in views)
    return math.sqrt(s) / div


# ---- the norm and scale kernels ----------------------------------------------------------------------
@pytest.mark.parametrize("div", [1.0, 3.0])
@pytest.mark.parametrize("name", list(CASES))
def test_norm_and_scale_kernels(device, name, div):
    buf, views, guard = _make(name, device)
    before = buf.clone()
    ref = _ref_norm(views, div)
    clip = GradClip(device, capacity=len(views))
    clip.bind(views)
    clip.run(INF, div)
    st = clip.read()
    print(f"{name} div={div}: norm {st['norm']!r} ref {ref!r} ulp {_ulp(ref)!r}")
    assert abs(st["norm"] - ref) <= _ulp(ref)
    assert st["coef"] == 1.0 and st["steps"] == 1 and st["clipped"] == 0
    assert torch.equal(_bits(buf), _bits(before))  # measure only: nothing written

    thr = float(np.float32(st["norm"] / 2))
    clip.run(thr, div)
    st2 = clip.read()
    assert st2["norm"] == st["norm"] and st2["steps"] == 2 and st2["clipped"] == 1
    coef = np.float32(thr) / (np.float32(st["norm"]) + np.float32(1e-6))
    assert st2["coef"] == float(coef) and 0.0 < st2["coef"] < 1.0
    want = torch.where(guard, before, before * st2["coef"])  # the product formed in torch fp32
    assert torch.equal(_bits(buf), _bits(want))
    assert torch.equal(buf[guard], torch.full_like(buf[guard], GUARD))


@pytest.mark.parametrize("n", [64 * 2048, 64 * 2048 + 1, BIG])
def test_ticket_group_boundaries(device, n):
    """One-entry tables of 64, 65 and 133 blocks (ticket groups of 64; 64 + 1; 64 + 64 + 5), three
    runs in a row on one GradClip: a first- or top-level counter that was not re-armed loses the
    second run's last arriver (stale block, steps short) or leaves a nonzero word behind."""
    v = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(device)
    ref = _ref_norm([v], 1.0)
    clip = GradClip(device, capacity=1)
    clip.bind([v])
    assert clip.plan.n_blocks == (n + 2047) // 2048
    norms = []
    for run in range(3):
        clip.run(INF)
        norms.append(clip.clip[0:1].clone())
        st = clip.read()
        print(f"n={n} run {run}: norm {st['norm']!r} ref {ref!r} ulp {_ulp(ref)!r}")
        assert abs(st["norm"] - ref) <= _ulp(ref)
        assert st["steps"] == run + 1 and st["coef"] == 1.0 and st["clipped"] == 0
    assert torch.equal(norms[0], norms[1]) and torch.equal(norms[0], norms[2])  # int32 words: bitwise
    assert clip.read()["steps"] == 3
    assert not clip.ctr.any().item(), "a ticket word was left nonzero"


def test_one_shot_front_end(device):
    buf, views, _ = _make("mix", device, seed=3)
    ref = _ref_norm(views, 1.0)
    before = [v.clone() for v in views]
    norm = ops.clip_grad_norm_(views, ref / 4)
    assert norm.is_cuda and norm.dtype == torch.float32 and abs(float(norm) - ref) <= _ulp(ref)
    coef = np.float32(ref / 4) / (np.float32(float(norm)) + np.float32(1e-6))
    for v, b in zip(views, before):
        assert torch.equal(v, b * float(coef))
    assert float(ops.clip_grad_norm_([], 1.0)) == 0.0
    with pytest.raises(ValueError):
        ops.clip_grad_norm_([views[3].double()], 1.0)       # not fp32: an error, never a fallback
    with pytest.raises(ValueError):
        ops.clip_grad_norm_([buf[: 64].view(8, 8).t()], 1.0)  # not contiguous


def test_minus_zero_survives_measuring(device):
    buf, views, _ = _make("mix", device, seed=4)
    for v in views:
        v[0] = -0.0
    before = buf.clone()
    clip = GradClip(device, capacity=len(views))
    clip.bind(views)
    clip.run(INF)
    assert clip.read()["coef"] == 1.0
    assert torch.equal(_bits(buf), _bits(before)) and bool(torch.signbit(views[5][0]))


@pytest.mark.parametrize("max_norm", [INF, 1.0])
def test_nan_gradient(device, max_norm):
    """A NaN element gives a NaN norm and so, by the rule (and torch.clamp), a NaN coefficient at any
    threshold, ``inf`` included: every element becomes NaN, the guards stay."""
    buf, views, guard = _make("mix", device, seed=5)
    views[7][100] = float("nan")
    ps = [torch.nn.Parameter(torch.zeros_like(v)) for v in views]
    for p, v in zip(ps, views):
        p.grad = v.clone()
    tnorm = torch.nn.utils.clip_grad_norm_(ps, max_norm, error_if_nonfinite=False)
    clip = GradClip(device, capacity=len(views))
    clip.bind(views)
    clip.run(max_norm)
    st = clip.read()
    assert math.isnan(st["norm"]) and math.isnan(st["coef"]) and st["clipped"] == 1
    assert math.isnan(float(tnorm))
    for p, v in zip(ps, views):
        assert torch.isnan(v).all() and torch.isnan(p.grad).all()
    assert torch.equal(buf[guard], torch.full_like(buf[guard], GUARD))


def test_inf_gradient(device):
    buf, views, guard = _make("mix", device, seed=6)
    views[9][17] = INF
    ps = [torch.nn.Parameter(torch.zeros_like(v)) for v in views]
    for p, v in zip(ps, views):
        p.grad = v.clone()
    tnorm = torch.nn.utils.clip_grad_norm_(ps, 1.0, error_if_nonfinite=False)
    clip = GradClip(device, capacity=len(views))
    clip.bind(views)
    clip.run(1.0)
    st = clip.read()
    assert st["norm"] == INF and float(tnorm) == INF
    assert st["coef"] == 0.0 and not math.copysign(1.0, st["coef"]) < 0  # +0
    for i, (p, v) in enumerate(zip(ps, views)):
        assert torch.equal(torch.isnan(v), torch.isnan(p.grad))
        assert torch.equal(torch.signbit(v), torch.signbit(p.grad))
        fin = ~torch.isnan(v)
        assert (v[fin] == 0).all() and torch.equal(v[fin], p.grad[fin])
        assert int(torch.isnan(v).sum()) == (1 if i == 9 else 0)
    assert torch.equal(buf[guard], torch.full_like(buf[guard], GUARD))


def test_ten_runs_one_bit_pattern(device):
    buf, views, _ = _make("mix", device, seed=7)
    before = buf.clone()
    thr = _ref_norm(views, 3.0) / 3
    clip = GradClip(device, capacity=len(views))
    clip.bind(views)
    seen, outs = set(), []
    for _ in range(10):
        buf.copy_(before)
        clip.run(thr, 3.0)
        w = clip.clip.cpu()
        seen.add((int(w[0]), int(w[1])))
        outs.append(buf.clone())
    st = clip.read()
    assert len(seen) == 1 and st["steps"] == 10 and st["clipped"] == 10
    assert all(torch.equal(_bits(o), _bits(outs[0])) for o in outs)


def test_graph_replay(device):
    buf, views, _ = _make("mix", device, seed=8)
    base = buf.clone()
    thr = float(np.float32(_ref_norm(views, 1.0)))  # contents scaled by 2 and 3 are over it, by 0.25 under
    clip = GradClip(device, capacity=len(views))
    snap = clip.snapshot()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up: modules loaded, table uploaded
        clip.bind(views)
        clip.run(thr)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    clip.restore(snap)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        clip.bind(views)
        clip.run(thr)
    torch.cuda.synchronize()
    assert clip.read()["steps"] == 0  # a capture runs nothing
    clipped = 0
    for k, scale in enumerate((2.0, 0.25, 3.0)):
        buf.copy_(base * scale)
        eager_buf = buf.clone()
        spans, _ = _layout(*CASES["mix"][:2])
        eager_views = [eager_buf[o: o + n] for o, n in spans]
        eager = GradClip(device, capacity=len(views))
        eager.bind(eager_views)
        eager.run(thr)
        g.replay()
        torch.cuda.synchronize()
        st, se = clip.read(), eager.read()
        clipped += int(scale > 1)
        assert np.float32(st["norm"]).tobytes() == np.float32(se["norm"]).tobytes()
        assert np.float32(st["coef"]).tobytes() == np.float32(se["coef"]).tobytes()
        assert (st["coef"] != 1.0) == (scale > 1)
        assert st["steps"] == k + 1 and st["clipped"] == clipped
        assert torch.equal(_bits(buf), _bits(eager_buf))


def test_growing_inside_a_capture_is_refused(device):
    clip = GradClip(device, capacity=1, blocks=1)
    big = torch.ones(3 * 2048, device=device)
    clip.bind([big[:8]])  # an eager bind first: one block, and the pinned upload pool exists
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(AssertionError, match="before graph capture"):
        with torch.cuda.graph(g):
            clip.bind([big])
    torch.cuda.synchronize()


# ---- PowerSGDOptimizer (the parameter set of tests/test_hyper_gpu.py) ----------------------------------
CENTRE, CORNER = 1 << 4, 0b110110000  # {4} and {4, 5, 7, 8}
SHAPES = [((130, 64, 3, 3), CENTRE),   # three Q row chunks, two P column chunks, n % 16 != 0
          ((18, 16, 3, 3), CORNER),
          ((32, 5, 3, 3), CENTRE),     # full width 45: the scalar (non-vector) paths
          ((32, 16, 3, 3), None),      # one full matrix
          ((50,), None)]               # a 1-D parameter
LR0 = 0.05


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


def _grads(gen, device, scale):
    out = []
    for s, mask in SHAPES:
        g = torch.randn(s, generator=gen) * scale
        g[_dead(s, mask)] = 0.0  # exact zeros in the dead taps
        out.append(g.to(device))
    return out


@pytest.fixture(scope="module")
def grad_steps():
    """The gradients of 4 steps of different size, drawn once and shared (every step clones them)."""
    gen = torch.Generator(device="cpu").manual_seed(5)
    dev = torch.device("cuda", 0)
    return [_grads(gen, dev, s) for s in (1.0, 0.25, 2.0, 0.5)] if torch.cuda.is_available() else []


def _opt(device, rank, lazy=True, **kw):
    ps = _params(device)
    o = PowerSGDOptimizer(ps, lr=LR0, momentum=0.9, rank=rank, **kw)
    if not lazy:
        o.lazy_ef = False
    return ps, o


def _step(ps, o, grads, coef=None):
    o.zero_grad()
    for p, g in zip(ps, grads):
        p.grad = g.clone() if coef is None or coef == 1.0 else g * coef  # one fp32 multiply in torch
    o.step()


def _same(oa, ob, what=""):
    assert torch.equal(oa.x, ob.x), what
    assert torch.equal(oa.m, ob.m), what
    assert torch.equal(oa.buf.q_warm, ob.buf.q_warm), what
    assert torch.equal(oa.buf.comm_buf, ob.buf.comm_buf), what  # P-hat and the rank-1 payload
    assert torch.equal(oa.e, ob.e), what


@pytest.mark.parametrize("write_grad", [False, True])
@pytest.mark.parametrize("lazy", [True, False])
@pytest.mark.parametrize("rank", [4, 32])
def test_powersgd_clip_is_the_premultiplied_step(device, grad_steps, rank, lazy, write_grad):
    norms = [math.sqrt(sum(float(g.double().pow(2).sum()) for g in gs)) for gs in grad_steps]
    thr = float(np.float32(0.5 * (min(norms) + max(norms))))
    assert min(norms) < thr < max(norms)
    pa, oa = _opt(device, rank, lazy, write_grad=write_grad, max_grad_norm=thr)
    pb, ob = _opt(device, rank, lazy, write_grad=write_grad)
    assert oa.overlap is False and oa.clip is not None and ob.clip is None and ob.clip_stats() is None
    coefs = []
    for step, grads in enumerate(grad_steps):
        _step(pa, oa, grads)
        st = oa.clip_stats()
        assert abs(st["norm"] - norms[step]) <= _ulp(norms[step]) and st["steps"] == step + 1
        coefs.append(st["coef"])
        _step(pb, ob, grads, coef=st["coef"])
        if write_grad:
            for a, b in zip(pa, pb):
                assert torch.equal(a.grad, b.grad), step
        _same(oa, ob, step)
    assert [c != 1.0 for c in coefs] == [n > thr for n in norms]
    assert oa.clip_stats()["clipped"] == sum(n > thr for n in norms) and 0 < oa.clip_stats()["clipped"] < 4
    oa.check_errors()


@pytest.mark.parametrize("write_grad", [False, True])
@pytest.mark.parametrize("lazy", [True, False])
@pytest.mark.parametrize("rank", [4, 32])
def test_powersgd_measuring_is_the_plain_step(device, grad_steps, rank, lazy, write_grad):
    pa, oa = _opt(device, rank, lazy, write_grad=write_grad, max_grad_norm=INF)
    pb, ob = _opt(device, rank, lazy, write_grad=write_grad)
    for step, grads in enumerate(grad_steps):
        _step(pa, oa, grads)
        _step(pb, ob, grads)
        _same(oa, ob, step)
    st = oa.clip_stats()
    assert st["steps"] == 4 and st["clipped"] == 0 and st["coef"] == 1.0 and st["norm"] > 0
    assert [lay is not None for lay in oa.buf.layout] == [lay is not None for lay in ob.buf.layout]
    oa.check_errors()  # the dead-tap flag did not fire
    assert oa.buf.orth_error() == 0


def test_powersgd_overlap_with_clip_raises(device):
    with pytest.raises(ValueError, match="overlap.*max_grad_norm"):
        PowerSGDOptimizer(_params(device), lr=LR0, rank=4, overlap=True, max_grad_norm=1.0)
    o = PowerSGDOptimizer(_params(device), lr=LR0, rank=4, max_grad_norm=1.0)
    with pytest.raises(ValueError, match="overlap.*max_grad_norm"):
        o.set_overlap(True)


def test_powersgd_clip_in_a_captured_step(device, grad_steps):
    norms = [math.sqrt(sum(float(g.double().pow(2).sum()) for g in gs)) for gs in grad_steps]
    thr = float(np.float32(0.5 * (min(norms) + max(norms))))
    pe, oe = _opt(device, 4, max_grad_norm=thr)
    for grads in grad_steps:
        _step(pe, oe, grads)
    pg, og = _opt(device, 4, max_grad_norm=thr)
    static = [g.clone() for g in grad_steps[0]]

    def pre():
        og.zero_grad()
        for p, s in zip(pg, static):
            p.grad = s.clone()
    runner = StepRunner(pre, og, mode="full", warmup=2)
    for grads in grad_steps:
        for s, g in zip(static, grads):
            s.copy_(g)
        runner()
    runner.join()
    torch.cuda.synchronize()
    _same(og, oe)
    assert og.clip_stats() == oe.clip_stats() and og.clip_stats()["steps"] == 4  # the warm-up left no trace
    og.check_errors()


# ---- BucketedDataParallel --------------------------------------------------------------------------------
def _mlp(device):
    torch.manual_seed(2)
    return torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.Tanh(), torch.nn.Linear(19, 23), torch.nn.Tanh(),
                               torch.nn.Linear(23, 5)).to(device)


def _ddp_run(device, mode, max_grad_norm, xs, coefs=None):
    """4 steps of a 3-layer MLP; ``coefs``: multiply every gradient by that step's coefficient in torch
    before the (unclipped) step.  Returns (ddp, the clip block after every step)."""
    model = _mlp(device)
    ddp = BucketedDataParallel(model, lr=0.1, momentum=0.9, max_grad_norm=max_grad_norm)
    x = xs[0].clone()
    coef = torch.ones((), device=device)

    def pre():
        ddp.zero_grad()
        model(x).square().mean().backward()
        if coefs is not None:
            for p in model.parameters():
                p.grad.mul_(coef)
    runner = StepRunner(pre, ddp, mode="full" if mode == "graph" else "none", warmup=2)
    stats = []
    for k, xk in enumerate(xs):
        x.copy_(xk)
        if coefs is not None:
            coef.fill_(coefs[k])
        runner()
        runner.join()
        stats.append(ddp.clip_stats())
    torch.cuda.synchronize()
    return ddp, stats


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_bucketed_data_parallel_clip(device, mode):
    gen = torch.Generator().manual_seed(9)
    xs = [(torch.randn(16, 37, generator=gen) * s).to(device) for s in (1.0, 3.0, 0.5, 2.0)]
    plain, none = _ddp_run(device, mode, 0.0, xs)
    assert none == [None] * 4
    meas, stats = _ddp_run(device, mode, INF, xs)
    assert torch.equal(meas.x, plain.x) and torch.equal(meas.buf, plain.buf)
    assert [s["steps"] for s in stats] == [1, 2, 3, 4] and stats[-1]["clipped"] == 0
    norms = [s["norm"] for s in stats]
    thr = float(np.float32(0.5 * (min(norms) + max(norms))))
    assert min(norms) < thr < max(norms)
    clipped, cstats = _ddp_run(device, mode, thr, xs)
    assert 0 < cstats[-1]["clipped"] < 4 and [s["steps"] for s in cstats] == [1, 2, 3, 4]
    twin, _ = _ddp_run(device, mode, 0.0, xs, coefs=[s["coef"] for s in cstats])
    assert torch.equal(clipped.x, twin.x) and torch.equal(clipped.buf, twin.buf)
    assert not torch.equal(clipped.x, plain.x)
    pad = torch.ones(clipped.numel, dtype=torch.bool, device=device)
    for p in clipped.params:
        o = clipped.offsets[id(p)]
        pad[o: o + p.numel()] = False
    assert (clipped.g[pad] == 0).all()  # the arena's padding is zero and stays zero


# ---- the engine ----------------------------------------------------------------------------------------------
def _engine_run(tmp_path, name, **over):
    torch.manual_seed(0)  # the engine builds the model from the current RNG
    cfg = engine.default_config(**dict(dict(verbose=False, log_file=str(tmp_path / f"{name}.jsonl")), **over))
    out = engine.run_task(cfg)
    recs = [json.loads(ln) for ln in (tmp_path / f"{name}.jsonl").read_text().splitlines()]
    return out, [r for r in recs if r["kind"] == "step"]


@pytest.mark.parametrize("grad_sync", ["powersgd", "dense"])
def test_engine_mlp_graph_against_eager(device, tmp_path, grad_sync):
    base = dict(task="mlp", grad_sync=grad_sync, training_epochs=2, dataset_size=256, global_batch=64,
                learning_rate=0.05)
    _, probe = _engine_run(tmp_path, "probe", graph_mode="none", max_grad_norm=INF, **base)
    norms = [r["grad_norm"] for r in probe]
    thr = float(np.float32(0.5 * (min(norms) + max(norms))))
    assert len(norms) == 8 and min(norms) < thr < max(norms)
    out_g, steps_g = _engine_run(tmp_path, "graph", graph_mode="auto", max_grad_norm=thr, **base)
    out_e, steps_e = _engine_run(tmp_path, "eager", graph_mode="none", max_grad_norm=thr, **base)
    assert out_g["graph_mode"] == "full" and out_e["graph_mode"] == "none"
    print("graph", [r["grad_norm"] for r in steps_g], "eager", [r["grad_norm"] for r in steps_e])
    assert [r["grad_norm"] for r in steps_g] == [r["grad_norm"] for r in steps_e]
    assert [r["clip_coef"] for r in steps_g] == [r["clip_coef"] for r in steps_e]
    for a, b in zip(out_g["model"].parameters(), out_e["model"].parameters()):
        assert torch.equal(a, b)
    assert 0 < out_g["clipped_steps"] < 8 and out_g["clipped_steps"] == out_e["clipped_steps"]
    assert out_g["max_grad_norm"] == thr


@pytest.mark.parametrize("grad_sync", ["powersgd", "dense"])
def test_engine_resnet18_measuring_changes_nothing(device, tmp_path, grad_sync):
    base = dict(task="cifar", model="resnet18", num_classes=10, global_batch=32, dataset_size=128, training_epochs=1,
                grad_sync=grad_sync, graph_mode="auto")
    off, steps_off = _engine_run(tmp_path, "off", max_grad_norm=0.0, **base)
    inf, steps_inf = _engine_run(tmp_path, "inf", max_grad_norm=INF, **base)
    assert off["graph_mode"] == inf["graph_mode"] == "full"
    assert len(steps_inf) == 4 and [r["loss"] for r in steps_inf] == [r["loss"] for r in steps_off]
    for a, b in zip(off["model"].parameters(), inf["model"].parameters()):
        assert torch.equal(a, b)
    assert off["param_checksum"] == inf["param_checksum"]
    assert all(math.isfinite(r["grad_norm"]) and r["grad_norm"] > 0 and r["clip_coef"] == 1.0 for r in steps_inf)
    assert not any("grad_norm" in r for r in steps_off)
    assert inf["clipped_steps"] == 0 and "clipped_steps" not in off
