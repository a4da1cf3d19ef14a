"""The weight EMA on the device (csrc/ema.hip, ops/ema.py): every comparison is bitwise against the
test-only rule (tests/ema_rule.py), NaN compared by position.  tests/test_ema_cpu.py checks that
these inputs tell the rule from its fused variant, so a contracted kernel cannot pass here.

The optimiser tests use the parameter set and arms of tests/test_hyper_gpu.py (local copies of its
helpers)."""
import numpy as np
import pytest
import torch

from network_distributed_pytorch_amd import engine, ops
from network_distributed_pytorch_amd.ops import taps
from network_distributed_pytorch_amd.parallel.ddp import BucketedDataParallel
from network_distributed_pytorch_amd.parallel.powersgd import PowerSGDOptimizer
from network_distributed_pytorch_amd.utils.graph import StepRunner

from . import ema_cases as C
from . import ema_rule as R

pytestmark = pytest.mark.gpu

F = np.float32


def _np(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().view(-1).numpy()


class _Raw:
    """The two kernels over hand-placed live / shadow views (guard bands, chosen alignment)."""

    def __init__(self, cases, device, seed=C.SEED):
        self.cases = cases
        live, shadow, self.ls, self.ss = C.buffers(cases, seed)
        self.live0, self.shadow0 = live, shadow
        self.live = torch.from_numpy(live.copy()).to(device)
        self.shadow = torch.from_numpy(shadow.copy()).to(device)
        assert self.live.data_ptr() % 16 == 0 and self.shadow.data_ptr() % 16 == 0
        self.x = [self.live[a: a + c[0]] for c, a in zip(cases, self.ls)]
        self.s = [self.shadow[b: b + c[0]] for c, b in zip(cases, self.ss)]
        for c, x, s in zip(cases, self.x, self.s):
            assert (x.data_ptr() % 16, s.data_ptr() % 16) == (4 * c[1], 4 * c[2])
        self.plan = ops.SegPlan([(x, s, 1, 0, 1.0) for x, s in zip(self.x, self.s)], device)
        self.ent, self.prefix, self.n_ent, self.n_blocks = self.plan.table()
        assert self.n_blocks == sum((c[0] + 2047) // 2048 for c in cases)
        self.ctr = torch.zeros(ops.ext().grad_clip_ctr_words(self.n_blocks), dtype=torch.int32, device=device)
        self.block = torch.zeros(4, dtype=torch.int32, device=device)

    def update(self, decay, warmup):
        ops.ext().ema_update(self.ent, self.prefix, self.n_ent, self.n_blocks, self.ctr, self.block, decay, warmup)

    def swap(self):
        ops.ext().ema_swap(self.ent, self.prefix, self.n_ent, self.n_blocks)

    def read(self):
        w = self.block.cpu()
        f = w[:2].view(torch.float32)
        return np.float32(f[0].item()), np.float32(f[1].item()), int(w[2]), int(w[3])

    def check_guards_and_tickets(self):
        live, shadow = _np(self.live), _np(self.shadow)
        gl = C.guard_mask(self.cases, self.ls, live.size)
        gs = C.guard_mask(self.cases, self.ss, shadow.size)
        assert np.all(live[gl].view(np.uint32) == C.SENTINEL.view(np.uint32))
        assert np.all(shadow[gs].view(np.uint32) == C.SENTINEL.view(np.uint32))
        assert not self.ctr.any().item()  # every ticket re-armed
        return live, shadow


# ---- 1. kernel shapes ----------------------------------------------------------------------------
@pytest.mark.parametrize("cases", [C.main_table()] + [[(n, 0, 0)] for n in C.ONE_ENTRY],
                         ids=["table", "64-blocks", "65-blocks"])
def test_update_every_shape_and_alignment(device, cases):
    raw = _Raw(cases, device)
    ref = [raw.shadow0[b: b + c[0]].copy() for c, b in zip(cases, raw.ss)]
    for n in range(2):  # warm-up: w = 0.9, then 9/11
        if n == 1:  # the weights moved
            for i, (c, x) in enumerate(zip(cases, raw.x)):
                x.copy_(torch.from_numpy(R.gaussians(C.SEED + 5000 + i, c[0])).to(device))
        live_before = _np(raw.live).copy()
        d, w = R.rule_decay(0.999, n, True)
        raw.update(0.999, True)
        torch.cuda.synchronize()
        live, shadow = raw.check_guards_and_tickets()
        assert np.array_equal(live.view(np.uint32), live_before.view(np.uint32))  # the live tensors stay bitwise
        got = raw.read()
        assert (got[0].tobytes(), got[1].tobytes(), got[2], got[3]) == (d.tobytes(), w.tobytes(), n + 1, 0)
        for i, (c, a, b) in enumerate(zip(cases, raw.ls, raw.ss)):
            ref[i] = R.rule_update(live[a: a + c[0]], ref[i], w)
            assert R.same_bits(shadow[b: b + c[0]], ref[i]), (c, n)


def test_update_special_values(device):
    x, s = R.special_pairs()
    for off in ((0, 0), (1, 1), (0, 1)):  # vector path with a partial float4, scalar paths
        base_x, base_s = torch.zeros(64, device=device), torch.zeros(64, device=device)
        xv, sv = base_x[4 + off[0]: 4 + off[0] + x.size], base_s[4 + off[1]: 4 + off[1] + s.size]
        xv.copy_(torch.from_numpy(x).to(device))
        ema = ops.WeightEma([xv], 0.5, warmup=False)
        assert ema.shadow[0].data_ptr() % 16 == xv.data_ptr() % 16
        ema.shadow[0].copy_(torch.from_numpy(s).to(device))
        ema.update()
        got = _np(ema.shadow[0])
        assert R.same_bits(got, R.rule_update(x, s, F(0.5)))
        assert got[1] == 0 and not np.signbit(got[1])   # a shared -0 becomes +0
        assert np.isnan(got[4]) and np.isnan(got[5])     # x = s = inf gives NaN
        assert got[10] == F(2.5)                         # x == s keeps the shadow
        assert R.same_bits(_np(xv), x)


# ---- 2. block and schedule ------------------------------------------------------------------------
@pytest.mark.parametrize("decay,warmup", [(0.5, True), (0.5, False), (0.999, True), (0.999, False)])
def test_block_and_schedule(device, decay, warmup):
    shapes = [(4097,), (33, 5), (), (2048,)]
    xs = [torch.from_numpy(R.gaussians(C.SEED + i, int(np.prod(s, dtype=np.int64))).reshape(s)).to(device)
          for i, s in enumerate(shapes)]
    ema = ops.WeightEma(xs, decay, warmup=warmup)
    assert ema.read() == {"decay": 0.0, "weight": 0.0, "updates": 0}
    ref = [_np(x).copy() for x in xs]
    assert all(R.same_bits(_np(s), r) for s, r in zip(ema.shadow, ref))
    for n in range(12):
        for i, x in enumerate(xs):
            x.copy_(torch.from_numpy(R.gaussians(C.SEED + 100 * (n + 1) + i, x.numel()).reshape(tuple(x.shape))).to(device))
        d, w = R.rule_decay(decay, n, warmup)
        ema.update()
        assert ema.read() == {"decay": float(d), "weight": float(w), "updates": n + 1}
        ref = [R.rule_update(_np(x), r, w) for x, r in zip(xs, ref)]
        for s, r in zip(ema.shadow, ref):
            assert R.same_bits(_np(s), r), n
    snap = ema.snapshot()
    ema.update()
    ema.restore(snap)
    assert ema.read()["updates"] == 12 and all(R.same_bits(_np(s), r) for s, r in zip(ema.shadow, ref))
    sd = ema.state_dict(["a", "b", "c", "d"])
    other = ops.WeightEma([x.clone() for x in xs], decay, warmup=warmup)
    other.load_state_dict(sd)
    assert other.read() == ema.read() and all(torch.equal(a, b) for a, b in zip(other.shadow, ema.shadow))


def test_device_argument_checks(device):
    with pytest.raises(ValueError, match="float32"):
        ops.WeightEma([torch.zeros(3, dtype=torch.float16, device=device)], 0.5)
    with pytest.raises(ValueError, match="contiguous"):
        ops.WeightEma([torch.zeros(4, 4, device=device).t()], 0.5)
    with pytest.raises(ValueError, match="tensor on"):
        ops.WeightEma([torch.zeros(4, device=device), torch.zeros(4)], 0.5)


# ---- 3. graph replay ------------------------------------------------------------------------------
def _replayed(device):
    cases = [(2049, 0, 0), (5, 1, 1), (C.BIG, 0, 0)]
    live, _, ls, _ = C.buffers(cases)
    buf = torch.from_numpy(live.copy()).to(device)
    xs = [buf[a: a + c[0]] for c, a in zip(cases, ls)]
    ema = ops.WeightEma(xs, 0.5, warmup=True)
    ref = [_np(x).copy() for x in xs]
    ema.update()  # one eager run first: the replays start from updates = 1
    ref = [R.rule_update(_np(x), r, R.rule_decay(0.5, 0, True)[1]) for x, r in zip(xs, ref)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ema.update()
    assert ema.read()["updates"] == 1  # a capture runs nothing
    for k in range(5):
        for i, x in enumerate(xs):
            x.copy_(torch.from_numpy(R.gaussians(C.SEED + 77 * (k + 1) + i, x.numel())).to(device))
        g.replay()
        ref = [R.rule_update(_np(x), r, R.rule_decay(0.5, 1 + k, True)[1]) for x, r in zip(xs, ref)]
    torch.cuda.synchronize()
    d, w = R.rule_decay(0.5, 5, True)
    assert ema.read() == {"decay": float(d), "weight": float(w), "updates": 6}  # the tickets were re-armed
    assert not ema.ctr.any().item()
    for s, r in zip(ema.shadow, ref):
        assert R.same_bits(_np(s), r)
    return [_np(s).copy() for s in ema.shadow], ema.block.cpu()


def test_graph_replay_follows_the_device_block(device):
    a, blk_a = _replayed(device)
    b, blk_b = _replayed(device)
    assert torch.equal(blk_a, blk_b)
    assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(a, b))


# ---- 4. swap --------------------------------------------------------------------------------------
def test_swap_is_bitwise_and_an_involution(device):
    cases = C.main_table()[:-1] + [(6 * 2048 + 3, 0, 0)]
    raw = _Raw(cases, device)
    payload = torch.tensor([0x7fc12345, -4194303, -2147483648, 0x7f800000], dtype=torch.int32, device=device)
    raw.x[-1][:4].view(torch.int32).copy_(payload)        # NaN payloads, -0, inf: the words themselves move
    raw.s[-1][:4].view(torch.int32).copy_(payload.flip(0))
    live0, shadow0 = _np(raw.live).copy().view(np.uint32), _np(raw.shadow).copy().view(np.uint32)
    raw.swap()
    torch.cuda.synchronize()
    live, shadow = raw.check_guards_and_tickets()
    for c, a, b in zip(cases, raw.ls, raw.ss):
        assert np.array_equal(live.view(np.uint32)[a: a + c[0]], shadow0[b: b + c[0]]), c
        assert np.array_equal(shadow.view(np.uint32)[b: b + c[0]], live0[a: a + c[0]]), c
    raw.swap()
    torch.cuda.synchronize()
    live, shadow = raw.check_guards_and_tickets()
    assert np.array_equal(live.view(np.uint32), live0) and np.array_equal(shadow.view(np.uint32), shadow0)
    assert raw.read()[2] == 0  # the block is not the swap's business


# ---- 5. in the syncs ------------------------------------------------------------------------------
CENTRE, CORNER = 1 << 4, 0b110110000  # {4} and {4, 5, 7, 8}
SHAPES = [((130, 64, 3, 3), CENTRE), ((18, 16, 3, 3), CORNER), ((32, 5, 3, 3), CENTRE), ((32, 16, 3, 3), None),
          ((50,), None)]
LR0, DECAY, STEPS = 0.05, 0.9, 4


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
    """The gradients of the steps, drawn once and shared (never modified: every step clones them)."""
    gen = torch.Generator(device="cpu").manual_seed(5)
    dev = torch.device("cuda", 0)
    return [_grads(gen, dev) for _ in range(STEPS)] if torch.cuda.is_available() else []


class _Holder(torch.nn.Module):
    def __init__(self, ps):
        super().__init__()
        self.ps = torch.nn.ParameterList(ps)


def _make(device, kind, rank, kw):
    ps = _params(device)
    if kind == "dense":
        return ps, BucketedDataParallel(_Holder(ps), lr=LR0, momentum=0.9)
    return ps, PowerSGDOptimizer(ps, lr=LR0, momentum=0.9, rank=rank, **kw)


def _state(kind, o):
    if kind == "dense":
        return [o.x.clone(), o.buf.clone()]
    return [o.x.clone(), o.m.clone(), o.buf.q_warm.clone()]


def _graph_run(device, kind, rank, kw, grad_steps, with_ema):
    ps, o = _make(device, kind, rank, kw)
    ema = None
    if with_ema:
        ema = ops.WeightEma([p.detach() for p in ps], DECAY)
        o.attach_ema(ema)
    static = [g.clone() for g in grad_steps[0]]

    def pre():
        o.zero_grad()
        for p, s in zip(ps, static):
            p.grad = s.clone()
    runner = StepRunner(pre, o, mode="full", warmup=2)
    for grads in grad_steps:
        for s, g in zip(static, grads):
            s.copy_(g)
        runner()
    runner.join()
    torch.cuda.synchronize()
    assert runner.replays == STEPS and bool(runner.side_graphs) == bool(kw.get("overlap"))
    return ps, o, ema


@pytest.mark.parametrize("kind,rank,kw", [("powersgd", 4, {}), ("powersgd", 4, dict(overlap=True, groups=2)),
                                          ("powersgd", 32, {}), ("dense", 0, {})],
                         ids=["r4", "r4-overlap", "r32", "dense"])
def test_ema_in_the_captured_step(device, grad_steps, kind, rank, kw):
    # eager, no EMA: the parameters after each step feed the rule
    pe, oe = _make(device, kind, rank, kw)
    ref = [_np(p).copy() for p in pe]
    for n, grads in enumerate(grad_steps):
        oe.zero_grad()
        for p, g in zip(pe, grads):
            p.grad = g.clone()
        oe.step()
        torch.cuda.synchronize()
        w = R.rule_decay(DECAY, n, True)[1]
        ref = [R.rule_update(_np(p), r, w) for p, r in zip(pe, ref)]
    _, o_off, _ = _graph_run(device, kind, rank, kw, grad_steps, False)
    ps, o_on, ema = _graph_run(device, kind, rank, kw, grad_steps, True)
    for a, b in zip(_state(kind, o_on), _state(kind, o_off)):
        assert torch.equal(a, b)  # the EMA never perturbs training
    assert torch.equal(o_on.x, oe.x)
    d, w = R.rule_decay(DECAY, STEPS - 1, True)
    assert ema.read() == {"decay": float(d), "weight": float(w), "updates": STEPS}  # warm-up left no trace
    for s, r in zip(ema.shadow, ref):
        assert R.same_bits(_np(s), r)
    if kind == "powersgd":
        o_on.check_errors()


# ---- 6. the engine ----------------------------------------------------------------------------------
def _engine_run(ckpt_dir, **over):
    cfg = engine.default_config(**dict(dict(
        task="cifar", model="resnet18", num_classes=10, dataset_size=64, global_batch=16, eval_size=32,
        training_epochs=2, graph_mode="auto", verbose=False, ema_decay=0.9, eval_every=1,
        checkpoint_dir=str(ckpt_dir)), **over))
    torch.manual_seed(0)  # the engine builds the model from the current RNG
    return cfg, engine.run_task(cfg)


@pytest.fixture(scope="module")
def engine_run(tmp_path_factory):
    """One ResNet-18 run with the EMA evaluated after both epochs, shared by the two tests below."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    ckpt = tmp_path_factory.mktemp("ema_engine")
    cfg, out = _engine_run(ckpt)
    assert out["graph_mode"] != "none" and out["ema_updates"] == out["steps"] == 8
    return cfg, out, ckpt


def test_engine_ema_loss_is_the_checkpointed_shadows(device, engine_run):
    from network_distributed_pytorch_amd.models import build_model
    from network_distributed_pytorch_amd.utils.config import validate_config

    cfg, out, ckpt = engine_run
    last = out["eval"][-1]
    state = torch.load(ckpt / "last.pt", map_location="cpu", weights_only=True)
    assert state["ema"]["updates"] == 8
    fresh = build_model("resnet18", 10).to(device)
    fresh.load_state_dict(state["ema"]["shadow"], strict=False)
    validate_config(cfg, strict=False)
    val = engine._build_data(cfg, device, 1, 0)[2]
    rec = engine.evaluate(fresh, val, batch=16, graph_mode=out["graph_mode"])
    print(f"ema_loss {last['ema_loss']!r} fresh {rec['loss']!r} live {last['loss']!r}")
    assert rec["loss"] == last["ema_loss"] and rec["top1"] == last["ema_top1"] and rec["topk"] == last["ema_topk"]
    assert last["ema_loss"] != last["loss"]


def test_engine_swap_leaves_training_untouched(device, engine_run, tmp_path):
    """The same run without evaluation ends on the same weights and shadow: the swap restored the
    weights, and the steps after it saw no stale weight-derived tensor (Winograd / Toeplitz banks)."""
    _, out, _ = engine_run
    _, plain = _engine_run(tmp_path, eval_every=0)
    print(f"checksum with eval {out['param_checksum']!r} without {plain['param_checksum']!r}")
    assert plain["param_checksum"] == out["param_checksum"]
    for a, b in zip(out["ema"].shadow, plain["ema"].shadow):
        assert torch.equal(a, b)
