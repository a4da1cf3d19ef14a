"""Scaled-sign compression on the device (csrc/signsgd.hip) against a plain reference written here:
per block an fp64 ``abs().sum()`` over torch's fp32 ``g + e``, a sign test, and the bits placed
through the documented ``word(t), bit(t)``; the update against the twin and an fp64 evaluation.
"""
import numpy as np
import pytest
import torch

from network_distributed_pytorch_amd.models.mlp import ToyMLP
from network_distributed_pytorch_amd.ops.signsgd import SignCore
from network_distributed_pytorch_amd.parallel.comm import Communicator
from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync

from . import psgd_rule as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
G = 2048
SEGSETS = ([1], [31], [32], [33], [63], [64], [65], [2047], [2048], [2049], [5, 2048, 33, 4097])
SENTINEL = 12345.0


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _layout(counts):
    """Segments at 16-aligned offsets with a gap before, between and behind them; the blocks."""
    segs, o = [], 16
    for c in counts:
        segs.append((o, c))
        o += (c + 15) // 16 * 16 + 16
    blocks = [(off + t, min(G, c - t)) for off, c in segs for t in range(0, c, G)]
    live = torch.zeros(o, dtype=torch.bool)
    for off, c in segs:
        live[off: off + c] = True
    return segs, blocks, o, live


def _inputs(arm, n, blocks):
    gen = torch.Generator().manual_seed(n)
    if arm == "gauss":
        return torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    g, e = (torch.randint(-1, 2, (n,), generator=gen).float() for _ in range(2))  # m in {-2 .. 2}
    g[::7], e[::7] = -0.0, -0.0  # m = -0: sends bit 1
    if arm == "special":  # in a block of small integers any fp64 order still gives the same sum
        for j, (off, ln) in enumerate(blocks):
            kind = (j + ln) % 4
            if kind == 0:
                g[off + ln // 2], e[off + ln // 2] = float("nan"), 0.0
            elif kind == 1:
                g[off + ln - 1], e[off + ln - 1] = float("inf"), 0.0
            elif kind == 2:
                g[off], e[off] = -float("inf"), 1.0
            else:
                for t, v in ((0, 1e-40), (3, -3e-39), (ln - 1, 2e-45)):
                    if t < ln:
                        g[off + t], e[off + t] = v, -0.0
    return g, e


def _place(j, t):
    return 64 * j + 8 * (t >> 8) + 2 * (t & 3) + ((t >> 7) & 1), (t >> 2) & 31


def _reference(g, e, blocks):
    """(sign words as int64 in [0, 2^32), scales fp32, m)"""
    m = g + e
    neg = m.view(torch.int32) < 0
    words = torch.zeros(64 * len(blocks), dtype=torch.int64)
    scales = []
    for j, (off, ln) in enumerate(blocks):
        t = torch.arange(ln)[neg[off: off + ln]]
        w, b = _place(j, t)
        words.index_add_(0, w, torch.ones_like(b) << b)
        scales.append((m[off: off + ln].double().abs().sum() / ln).float())
    return words, torch.stack(scales), m


def _residual(m, e0, scales, blocks):
    res = e0.clone()
    for (off, ln), s in zip(blocks, scales):
        mb = m[off: off + ln]
        res[off: off + ln] = mb - torch.where(mb.view(torch.int32) < 0, -s.abs(), s.abs())
    return res


def _nan_canon(t):
    """IEEE 754 leaves the sign of a NaN result open: for m - c with c NaN the host keeps c's sign and
    gfx950 flips it (measured: 0x7fc00000 against 0xffc00000).  Against the plain reference NaNs
    compare as NaNs and every other value bit for bit; against the twin everything is bit for bit."""
    return _bits(torch.where(torch.isnan(t.cpu()), torch.full((), float("nan")), t.cpu()))


@pytest.mark.parametrize("arm", ["int", "gauss", "special"])
@pytest.mark.parametrize("counts", SEGSETS, ids=lambda c: "-".join(map(str, c)))
def test_compress_is_the_plain_reference(counts, arm):
    """``int`` / ``special``: every fp64 sum of a block is exact in any order, so words, scales and e'
    are the reference's bit for bit.  ``gauss``: an fp64 sum of at most 2048 non-negative terms has a
    relative error below 2048 * 2^-53 = 2^-42 in any order, far below half an fp32 ulp (2^-24), so the
    two fp32 roundings of the two sums land on the same float or on neighbours: one ulp; e' is then
    bitwise m - c for the scale the kernel sent."""
    segs, blocks, n, live = _layout(counts)
    nb = len(blocks)
    g, e0 = _inputs(arm, n, blocks)
    e0[~live] = SENTINEL
    words, scales, m = _reference(g, e0, blocks)
    core = SignCore(DEV, segs, n)
    assert (core.nb, core.words, core.block) == (nb, 65 * nb, G)
    twin_e = e0.clone()
    twin = SignCore("cpu", segs, n).compress(g, twin_e)
    for call in range(2):
        ed = e0.clone().to(DEV)
        out = core.compress(g.to(DEV), ed).cpu()
        sent = out[64 * nb:].view(torch.float32)
        assert torch.equal(out[: 64 * nb].long() & 0xFFFFFFFF, words), call
        if arm == "gauss":
            assert (out[64 * nb:] - _bits(scales)).abs().max() <= 1, call
        else:
            assert torch.equal(out[64 * nb:], _bits(scales)), (call, out[64 * nb:], _bits(scales))
        assert torch.equal(_nan_canon(ed), _nan_canon(_residual(m, e0, sent, blocks))), call
        assert torch.equal(out, twin) and torch.equal(_bits(ed), _bits(twin_e)), call
        assert torch.equal(_bits(ed)[~live], _bits(e0)[~live]), call


UPD_COUNTS = [5, 2048, 33, 4097]


def _decode(row, blocks, n):
    """The arena of c (zero outside the blocks) and of |c| one wire buffer holds, in fp32."""
    nb, c = len(blocks), torch.zeros(n)
    for j, (off, ln) in enumerate(blocks):
        w, b = _place(j, torch.arange(ln))
        s = (row[64 * nb + j: 64 * nb + j + 1] & 0x7FFFFFFF).view(torch.float32)
        c[off: off + ln] = torch.where(((row[w] >> b.int()) & 1) == 1, -s, s)
    return c


@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_update_is_the_twin_and_within_the_rounding_bound(N, wd):
    """Bound (tests/test_topk_gpu.py derives it): x' passes through at most K = (N - 1) + 6 fp32
    roundings, each of relative size 2^-24 of a term of S, the same rule on absolute values without
    rounding; |dev - fp64| <= (K + 2) 2^-24 S, the 2 covering second-order terms and the reference's
    own fp64 error.  b' has two roundings fewer."""
    segs, blocks, n, live = _layout(UPD_COUNTS)
    nb, lr, lam = len(blocks), 0.05, 0.9
    gen = torch.Generator().manual_seed(N)
    x, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    x[~live], b[~live] = SENTINEL, -SENTINEL
    gathered = torch.cat([torch.randint(-2 ** 31, 2 ** 31, (N, 64 * nb), generator=gen).to(torch.int32),
                          torch.rand(N, nb, generator=gen).view(torch.int32)], 1).contiguous()
    core = SignCore(DEV, segs, n, N)
    xt, bt = x.clone(), b.clone()
    SignCore("cpu", segs, n, N).update(xt, bt, gathered, lr, lam, wd)
    runs = [torch.tensor([lr, wd, 0.0, 0.0], device=DEV)] + ([None] if wd == 0 else [])  # lr by value too
    for hy in runs:
        xd, bd = x.clone().to(DEV), b.clone().to(DEV)
        core.update(xd, bd, gathered.to(DEV), lr if hy is None else 0.0, lam, 0.0, hy)
        assert torch.equal(_bits(xd), _bits(xt)) and torch.equal(_bits(bd), _bits(bt))
    if wd:
        with pytest.raises(ValueError, match="hyper block"):
            core.update(xd, bd, gathered.to(DEV), lr, lam, wd, None)
    assert torch.equal(_bits(xd)[~live], _bits(x)[~live]) and torch.equal(_bits(bd)[~live], _bits(b)[~live])
    cs = [_decode(row, blocks, n) for row in gathered]
    acc64, mag = sum(c.double() for c in cs), sum(c.double().abs() for c in cs)
    f32 = [float(np.float32(v)) for v in (lr, lam, wd)]
    d64 = f32[2] * x.double() + acc64 / N
    b64 = b.double() * f32[1] + d64
    x64 = x.double() - f32[0] * (d64 + b64)
    _, bS, _, xS = R.element_step(R._Ops(True), mag / N, b.double().abs(), x.double().abs(), *f32)
    assert ((xd.cpu().double() - x64).abs() <= (N + 7) * R.EPS32 * xS)[live].all()
    assert ((bd.cpu().double() - b64).abs() <= (N + 5) * R.EPS32 * bS)[live].all()


def _sync(device):
    torch.manual_seed(0)
    model = ToyMLP().to(device)
    return model, build_grad_sync("signsgd", model, Communicator(), lr=0.05, momentum=0.9)


def _grads(model, step):
    """The CPU model's gradients of one seeded batch (both replicas are fed these very values)."""
    gen = torch.Generator().manual_seed(step)
    x, y = torch.randn(16, 32, generator=gen), torch.randint(0, 4, (16,), generator=gen)
    model.zero_grad()
    torch.nn.functional.cross_entropy(model(x), y).backward()
    return [p.grad.clone() for p in model.parameters()]


def _state(sync):
    return [_bits(t) for t in (sync.x, sync.buf, sync.e)]


def test_sync_on_the_device_is_the_cpu_twin_bitwise():
    cpu_model, cpu = _sync("cpu")
    dev_model, dev = _sync(DEV)
    for step in range(4):
        grads = _grads(cpu_model, step)
        cpu.zero_grad(), dev.zero_grad()
        for p, q, g in zip(cpu_model.parameters(), dev_model.parameters(), grads):
            p.grad, q.grad = g, g.to(DEV)
        assert cpu.step() == dev.step() == 8 * 4 * 65 * cpu.core.nb
        assert all(torch.equal(a, b) for a, b in zip(_state(cpu), _state(dev))), step
    assert cpu.e.any()


def test_captured_step_replays_like_the_eager_steps():
    model, _ = _sync("cpu")
    grads = [g.to(DEV) for g in _grads(model, 0)]
    states = []
    for captured in (False, True):
        dev_model, sync = _sync(DEV)
        for p, g in zip(dev_model.parameters(), grads):
            p.grad = g  # static gradient tensors: the flatten launch copies them into the arena
        if captured:
            snap, side = sync.snapshot(), torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                sync.step()  # warm-up: table uploads
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                sync.step()
            sync.restore(snap)
        for _ in range(3):
            graph.replay() if captured else sync.step()
        states.append(_state(sync))
    assert all(torch.equal(a, b) for a, b in zip(*states))
