"""Top-k sparsification on the device (csrc/topk.hip) against a plain reference written here.

Select: a stable sort of (key descending, index ascending), the first k, sorted by index; ``idx``,
``val`` and the residual ``e`` bitwise.  Update: per-rank sequential ``index_add`` in fp32 and the
element rule, bitwise against the twin, and within a derived bound of an fp64 evaluation.
"""
import numpy as np
import pytest
import torch

from network_distributed_pytorch_amd.models.mlp import ToyMLP
from network_distributed_pytorch_amd.ops.topk import TopKCore
from network_distributed_pytorch_amd.parallel.comm import Communicator
from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync

from . import psgd_rule as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
# the last size: 269 chunks, so more than one group of the two-level ticket and runs of two chunks
# per thread in the count launch's prefix (k = n / 100 only there, to stay quick)
SIZES = (1, 255, 2048, 2049, 3 * 2048 + 17, 70001, 2_200_003)
ARMS = ("gauss", "ties", "equal", "close", "special")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _inputs(arm, n):
    gen = torch.Generator().manual_seed(n)
    g, e = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    if arm == "ties":  # m in {0, +-1, +-2}: the tie rule and k - c decide
        g, e = (torch.randint(-1, 2, (n,), generator=gen).float() for _ in range(2))
    elif arm == "equal":
        g, e = torch.full((n,), 0.5), torch.full((n,), 0.25)
    elif arm == "close":  # 1 + j 2^-23: the first digit is shared, passes 1 and 2 do the work
        g = 1.0 + ((torch.arange(n) * 7919) % 3001).float() * 2.0 ** -23
        e = torch.zeros(n)
    elif arm == "special":
        vals = [1e-40, -3e-39, -0.0, float("inf"), -float("inf"), 2e-45, float("nan")]
        for j, v in enumerate(vals[: n]):
            g[(j * 9973 + 3) % n], e[(j * 9973 + 3) % n] = v, 0.0
    return g, e


def _select_ref(g, e, k):
    m = g + e
    key = m.view(torch.int32) & 0x7FFFFFFF
    idx = torch.sort(key, descending=True, stable=True).indices[:k].sort().values
    res = m.clone()
    res[idx] = 0.0
    return idx.to(torch.int32), m.view(torch.int32)[idx], res


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("n", SIZES)
def test_select_is_the_stable_sort_and_leaves_clean_scratch(n, arm):
    g, e = _inputs(arm, n)
    for k in sorted({1, max(1, n // 100), max(1, n - 1), n} if n < 10 ** 6 else {n // 100}):
        idx, val, res = _select_ref(g, e, k)
        core = TopKCore(DEV, n, k)
        for call in range(2):  # the second call finds the histogram zeroed and the tickets re-armed
            ed = e.to(DEV)
            out = core.select(g.to(DEV), ed).cpu()
            assert torch.equal(out[:k], idx), (k, call)
            assert torch.equal(out[k:], val), (k, call)
            assert torch.equal(_bits(ed), _bits(res)), (k, call)


UPD_N = 3 * 2048 + 17  # three full tiles (the third without entries) and a ragged one
UPD_IDX = ([0, 2047, 2048, 2049, 6144, 6160], [5, 2047, 2048, 3000, 6150, 6160], [2047, 2048, 4095, 6144, 6159, 6160])


@pytest.mark.parametrize("hyper", [False, True])
@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_update_is_the_twin_and_within_the_rounding_bound(N, wd, hyper):
    """Bound: x' passes through at most K = (N - 1) + 6 fp32 roundings (the rank adds after the first,
    which is exact, the division, the decay fma, fmul, two fadds and the last fma), each of relative
    size 2^-24 of a term of S, the same rule on absolute values without rounding; so
    |dev - fp64| <= (K + 2) 2^-24 S to first order, the 2 covering the second-order terms and the
    reference's own fp64 error.  b' has two roundings fewer."""
    n, k, lr, lam = UPD_N, len(UPD_IDX[0]), 0.05, 0.9
    gen = torch.Generator().manual_seed(N)
    x, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    gathered = torch.stack([torch.cat([torch.tensor(UPD_IDX[r], dtype=torch.int32),
                                       torch.randn(k, generator=gen).view(torch.int32)]) for r in range(N)])
    hy = torch.tensor([lr, wd, 0.0, 0.0], device=DEV) if hyper else None
    xd, bd = x.to(DEV), b.to(DEV)
    if wd and not hyper:  # the decay reaches the kernel through the block only
        with pytest.raises(ValueError, match="hyper block"):
            TopKCore(DEV, n, k, N).update(xd, bd, gathered.to(DEV), lr, lam, wd, None)
        return
    TopKCore(DEV, n, k, N).update(xd, bd, gathered.to(DEV), 0.0 if hyper else lr, lam, wd, hy)
    xt, bt = x.clone(), b.clone()
    TopKCore("cpu", n, k, N).update(xt, bt, gathered, lr, lam, wd)
    assert torch.equal(_bits(xd), _bits(xt)) and torch.equal(_bits(bd), _bits(bt))
    # plain reference: sequential index_add in fp32, then the rule through the fp32-rounding helpers
    acc, acc64, mag = torch.zeros(n), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for row in gathered:
        i, v = row[:k].long(), row[k:].view(torch.float32)
        acc.index_add_(0, i, v)
        acc64.index_add_(0, i, v.double())
        mag.index_add_(0, i, v.double().abs())
    o = acc / N if N != 1 else acc
    f32 = [float(np.float32(v)) for v in (lr, lam, wd)]
    _, mm, _, xx = R.element_step(R._Ops(False), o.double(), b.double(), x.double(), *f32)
    assert torch.equal(xx.float(), xt) and torch.equal(mm.float(), bt)
    d64 = f32[2] * x.double() + acc64 / N
    b64 = b.double() * f32[1] + d64
    x64 = x.double() - f32[0] * (d64 + b64)
    _, bS, _, xS = R.element_step(R._Ops(True), mag / N, b.double().abs(), x.double().abs(), *f32)
    assert ((xd.cpu().double() - x64).abs() <= (N + 7) * R.EPS32 * xS).all()
    assert ((bd.cpu().double() - b64).abs() <= (N + 5) * R.EPS32 * bS).all()


def _sync(device, ratio=0.25, seed=0):
    torch.manual_seed(seed)
    model = ToyMLP().to(device)
    return model, build_grad_sync("topk", model, Communicator(), lr=0.05, momentum=0.9, topk_ratio=ratio)


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
        assert cpu.step() == dev.step() == 64 * cpu.k
        assert all(torch.equal(a, b) for a, b in zip(_state(cpu), _state(dev))), step
    assert cpu.e.any() and cpu.k < cpu.numel


def test_captured_step_replays_like_the_eager_steps_and_ratio_one_keeps_no_error():
    model, _ = _sync("cpu")
    grads = [g.to(DEV) for g in _grads(model, 0)]
    states = []
    for captured in (False, True):
        dev_model, sync = _sync(DEV, ratio=1.0 if captured else 0.25)
        if captured:  # ratio 1 first: every non-zero entry is sent, nothing is fed back
            for p, g in zip(dev_model.parameters(), grads):
                p.grad = g
            sync.step()
            assert not sync.e.any()
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
