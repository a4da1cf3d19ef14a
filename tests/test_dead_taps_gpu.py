"""Dead-tap compaction of the PowerSGD error memory / momentum (ops/taps.py, csrc/powersgd.hip):
every step is bitwise the full layout's.  The compared arm is the same code with the
``dead_taps`` switch off, which runs the parent's plan byte for byte (tools/asan/plan_fuzz.cpp)."""
import pytest
import torch

from network_distributed_pytorch_amd.models.conv_gemm import GemmConv2d
from network_distributed_pytorch_amd.ops import taps
from network_distributed_pytorch_amd.parallel.powersgd import PowerSGDOptimizer
from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync
from network_distributed_pytorch_amd.utils.graph import StepRunner

pytestmark = pytest.mark.gpu

CENTRE, CORNER = 1 << 4, 0b110110000  # {4} and {4, 5, 7, 8}
# weight shape, live-tap mask (None: no support recorded)
SHAPES = [((130, 64, 3, 3), CENTRE),   # three Q row chunks, two P column chunks, n % 16 != 0
          ((18, 16, 3, 3), CORNER),
          ((32, 5, 3, 3), CENTRE),     # live width 5, full width 45: the scalar (non-vector) paths
          ((32, 16, 3, 3), None),      # one full matrix
          ((50,), None)]               # a 1-D parameter


def _dead(shape, mask):
    """bool [shape]: the dead-tap entries of a conv weight."""
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


def _grads(gen, device, poke=None):
    out = []
    for i, (s, mask) in enumerate(SHAPES):
        g = torch.randn(s, generator=gen)
        g[_dead(s, mask)] = 0.0  # exact zeros in the dead taps
        if poke is not None and i == poke:
            g[3, 2, 0, 0] = 0.5
        out.append(g.to(device))
    return out


def _opt(device, on, rank, lazy=True, **kw):
    ps = _params(device)
    o = PowerSGDOptimizer(ps, lr=0.05, momentum=0.9, rank=rank, **kw)
    o.dead_taps = on
    if not lazy:
        o.lazy_ef = False
    return ps, o


def _step(ps, o, grads):
    o.zero_grad()
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    o.step()


def _same(oa, ob, what=""):
    assert torch.equal(oa.x, ob.x), what
    assert torch.equal(oa.m, ob.m), what
    assert torch.equal(oa.buf.q_warm, ob.buf.q_warm), what
    assert torch.equal(oa.buf.comm_buf, ob.buf.comm_buf), what  # P-hat (and the rank-1 payload)
    assert torch.equal(oa.e, ob.e), what


@pytest.mark.parametrize("rank,lazy,kw", [
    (1, True, {}), (4, True, {}), (8, True, {}), (4, False, {}), (8, False, {}),
    (4, True, dict(overlap=True, groups=2)), (4, True, dict(write_grad=True)), (4, False, dict(write_grad=True)),
    (16, True, {}),  # still a wide plan (rank <= 16): compacted; above it see the next test
])
def test_reducer_compaction_bitwise(device, rank, lazy, kw):
    pa, oa = _opt(device, True, rank, lazy, **kw)
    pb, ob = _opt(device, False, rank, lazy, **kw)
    gen = torch.Generator(device="cpu").manual_seed(5)
    for step in range(4):
        grads = _grads(gen, device)
        _step(pa, oa, grads)
        _step(pb, ob, grads)
        if kw.get("write_grad"):
            for a, b in zip(pa, pb):
                assert torch.equal(a.grad, b.grad), step
        _same(oa, ob, step)
    compact = [lay is not None for lay in oa.buf.layout]
    assert compact == [True, True, True, False] and not any(lay is not None for lay in ob.buf.layout)
    assert oa.buf.compact_cols == [64, 64, 5, 144]
    if rank == 8:  # the wide plan's boundary: rank 8 still takes 512-column P items
        assert max(oa.buf.p_chunks) == 2 and max(oa.buf.q_chunks) == 3
    oa.check_errors()
    assert oa.bits_per_step == ob.bits_per_step and oa.collective_payloads() == ob.collective_payloads()


def test_rank_above_wide_kernels_stays_full(device):
    """Rank 32 plans run the narrow kernels, which know no compact layout: nothing is compacted."""
    pa, oa = _opt(device, True, 32)
    pb, ob = _opt(device, False, 32)
    gen = torch.Generator(device="cpu").manual_seed(5)
    for step in range(2):
        grads = _grads(gen, device)
        _step(pa, oa, grads)
        _step(pb, ob, grads)
        _same(oa, ob, step)
    assert all(lay is None for lay in oa.buf.layout)


def test_nonzero_dead_gradient_is_flagged(device):
    pa, oa = _opt(device, True, 4)
    gen = torch.Generator(device="cpu").manual_seed(5)
    _step(pa, oa, _grads(gen, device))
    oa.check_errors()
    _step(pa, oa, _grads(gen, device, poke=0))  # tap 0 of the centre-tap weight
    torch.cuda.synchronize()
    assert torch.isfinite(oa.x).all() and torch.isfinite(oa.m).all() and torch.isfinite(oa.e).all()
    with pytest.raises(RuntimeError, match="dead"):
        oa.check_errors()


@pytest.mark.parametrize("first_on", [True, False])
def test_checkpoint_interchange(device, first_on):
    gen = torch.Generator(device="cpu").manual_seed(8)
    steps = [_grads(gen, device) for _ in range(4)]
    pr, ref = _opt(device, False, 4)
    for g in steps:
        _step(pr, ref, g)
    pa, oa = _opt(device, first_on, 4)
    for g in steps[:2]:
        _step(pa, oa, g)
    assert any(lay is not None for lay in oa.buf.layout) == first_on
    sd = oa.state_dict()
    pb, ob = _opt(device, not first_on, 4)
    with torch.no_grad():
        for a, b in zip(pa, pb):
            b.copy_(a)
    ob.load_state_dict(sd)
    for g in steps[2:]:
        _step(pb, ob, g)
    assert any(lay is not None for lay in ob.buf.layout) == (not first_on)
    _same(ob, ref)
    # loading into an optimizer that is already compact goes through the full layout too
    oa.load_state_dict(sd)
    for g in steps[2:]:
        _step(pa, oa, g)
    _same(oa, ref)


def test_nonzero_dead_momentum_stays_full(device):
    gen = torch.Generator(device="cpu").manual_seed(8)
    steps = [_grads(gen, device) for _ in range(2)]
    outs = []
    for on in (True, False):
        ps, o = _opt(device, on, 4)
        sd = o.state_dict()
        s = o.offsets[id(ps[1])]
        sd["momentum"][s] = 0.25  # entry [0, 0, 0, 0] of the second weight: tap 0 is dead
        o.load_state_dict(sd)
        for g in steps:
            _step(ps, o, g)
        outs.append(o)
    assert [lay is not None for lay in outs[0].buf.layout] == [True, False, True, False]
    _same(outs[0], outs[1])


class _TwoConv(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.c1 = GemmConv2d(16, 32, 3, padding=1, bias=False)
        self.c2 = GemmConv2d(32, 32, 3, padding=1, bias=False)

    def forward(self, x):
        return self.c2(torch.relu(self.c1(x))).mean((2, 3))


def test_widening_decompacts(device):
    """2 steps on 1x1 maps (centre tap only), then 2x2 maps: every tap goes live, the plan returns
    to the full layout and the run equals one that never compacted."""
    gen = torch.Generator(device="cpu").manual_seed(2)
    xs = [torch.randn(8, 16, s, s, generator=gen).to(device) for s in (1, 1, 2)]
    ys = [torch.randint(0, 32, (8,), generator=gen).to(device) for _ in xs]
    outs = []
    for on in (True, False):
        torch.manual_seed(4)
        model = _TwoConv().to(device)
        o = PowerSGDOptimizer(model.parameters(), lr=0.05, momentum=0.9, rank=4)
        o.dead_taps = on
        for i, (x, y) in enumerate(zip(xs, ys)):
            o.zero_grad()
            torch.nn.functional.cross_entropy(model(x), y).backward()
            o.step()
            assert [lay is not None for lay in o.buf.layout] == [on and i < 2] * 2, i
        o.check_errors()
        outs.append(o)
    _same(outs[0], outs[1])


@pytest.mark.parametrize("mode,overlap", [("none", False), ("full", False), ("full", True)])
def test_resnet18_compaction_bitwise(device, mode, overlap):
    from network_distributed_pytorch_amd.models import build_resnet

    gen = torch.Generator(device="cpu").manual_seed(0)
    batches = [(torch.randn(8, 3, 32, 32, generator=gen).to(device), torch.randint(0, 10, (8,), generator=gen).to(device))
               for _ in range(3)]
    layer4 = ["layer4.0.conv1.weight", "layer4.0.conv2.weight", "layer4.1.conv1.weight", "layer4.1.conv2.weight"]
    masks = [CORNER, CENTRE, CENTRE, CENTRE]
    results = []
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        for on in (True, False):
            torch.manual_seed(3)
            model = build_resnet(18, 10).to(device)
            init = {k: v.detach().clone() for k, v in model.named_parameters()}
            sync = build_grad_sync("powersgd", model, lr=1e-2, momentum=0.9, rank=4, overlap=overlap)
            sync.opt.dead_taps = on
            static = [batches[0][0].clone(), batches[0][1].clone()]

            def pre():
                sync.zero_grad()
                torch.nn.functional.cross_entropy(model(static[0]), static[1]).backward()

            runner = StepRunner(pre, sync, mode=mode, warmup=2, state_tensors=list(model.buffers()))
            for x, y in batches:
                static[0].copy_(x)
                static[1].copy_(y)
                runner()
            torch.cuda.synchronize()
            sync.check_errors()
            names = [n for n, p in model.named_parameters() if p.dim() > 1]
            got = {names[i] for i, lay in enumerate(sync.opt.buf.layout) if lay is not None}
            assert got == (set(layer4) if on else set())
            results.append((dict(model.named_parameters()), dict(model.named_buffers()), init,
                            sync.bytes_per_step, sync.collective_payloads(), sync.opt.m, sync.opt.e))
    finally:
        torch.backends.cudnn.deterministic = det
    (pa, ba, init, bits_a, pay_a, ma, ea), (pb, bb, _, bits_b, pay_b, mb, eb) = results
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
    for k in ba:
        assert torch.equal(ba[k], bb[k]), k
    assert torch.equal(ma, mb) and torch.equal(ea, eb)
    assert bits_a == bits_b and pay_a == pay_b
    moved = 0
    for k, mask in zip(layer4, masks):  # the dead taps never move
        d = _dead(pa[k].shape, mask).to(device)
        assert torch.equal(pa[k][d], init[k][d]), k
        moved += int((pa[k][~d] != init[k][~d]).sum())
    assert moved > 0
