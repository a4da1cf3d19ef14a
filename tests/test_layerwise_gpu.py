"""LAMB / LARS on the device (csrc/layerwise.hip): every step against the plain reference and its bounds
(tests/layerwise_rule.py), LARS against the SGD launch, graph replay, and the two gradient-sync kinds."""
import numpy as np
import pytest
import torch

from network_distributed_pytorch_amd import ops
from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync

from . import layerwise_rule as L

pytestmark = pytest.mark.gpu
KINDS = ["lamb", "lars"]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("div", [1.0, 4.0])
@pytest.mark.parametrize("kind", KINDS)
def test_every_step_within_the_bounds(device, kind, div, wd):
    L.check_steps(device, kind, div, wd)


def test_lars_with_trust_one_is_the_sgd_launch(device):
    """Every tensor exempt (lam = 1) and wd = 0: bitwise ``sgd_momentum_`` over the same flat arenas."""
    opt, xs, gs, _ = L.make(device, "lars", 0.0, exempt_all=True)
    X, G = opt.flat
    X2, B2 = X.clone(), torch.zeros_like(X)
    for k in range(3):
        L.fill_grads(gs, k)
        opt.step(4.0)
        ops.sgd_momentum_(X2, G, B2, L.LR, L.MU, 4.0, hyper=opt.hyper.dev)
        assert torch.equal(_bits(X), _bits(X2))
        for x, b in zip(xs, opt.momentum_buffer):
            o = (x.data_ptr() - X.data_ptr()) // 4
            assert torch.equal(_bits(b), _bits(B2[o: o + x.numel()]))
    assert torch.all(opt.trust_ratios() == 1)


def _state(opt):
    arenas = [opt.flat[0], opt.m_arena] + ([opt.v_arena] if opt.core.lamb else [])
    return [_bits(t).clone() for t in arenas] + [opt.core.trust.clone()] + ([opt.core.block.clone()] if opt.core.lamb else [])


@pytest.mark.parametrize("kind", KINDS)
def test_graph_replay_is_the_eager_run(device, kind):
    """Three steps in one captured graph, replayed three times, against the same nine steps as eager
    launches: weights, moments, trust ratios and block bitwise (ticket re-arm, block advance, fixed
    summation order)."""
    opt, _, gs, _ = L.make(device, kind, 0.01)
    eager, _, egs, _ = L.make(device, kind, 0.01)
    L.fill_grads(gs, 0)
    L.fill_grads(egs, 0)
    snap, x0 = opt.snapshot(), opt.flat[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up: modules loaded, table uploaded
        opt.step(4.0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    opt.restore(snap)
    opt.flat[0].copy_(x0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(3):
            opt.step(4.0)
    torch.cuda.synchronize()
    for _ in range(3):
        graph.replay()
        for _ in range(3):
            eager.step(4.0)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(_state(opt), _state(eager)))
    assert (opt.read() or {}).get("steps") == (9 if kind == "lamb" else None)


def _mlp(device):
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(12, 16), torch.nn.ReLU(), torch.nn.Linear(16, 5)).to(device)


def _step(sync, seed):
    gen = torch.Generator().manual_seed(seed)
    sync.zero_grad()
    for p in sync.params:
        p.grad = (torch.randn(p.shape, generator=gen) * 0.1).to(p.device)
    sync.step()


@pytest.mark.parametrize("kind", KINDS)
def test_through_build_grad_sync(device, kind):
    cpu = torch.device("cpu")
    mk = lambda dev: build_grad_sync("dense-" + kind, _mlp(dev), lr=L.LR, momentum=L.MU, betas=(L.B1, L.B2),  # noqa: E731
                                     eps=L.EPS, lars_coef=L.ETA, lars_eps=L.EPS_L, decay_1d=False)
    dev, twin = mk(device), mk(cpu)
    for s in (dev, twin):
        s.set_hyper(L.LR, 0.01)
    for k in range(2):
        st = twin.adam_stats()
        block = (np.float32(st["b1pow"]), np.float32(st["b2pow"]), st["steps"]) if st else None
        pre = [t.numpy().copy() for t in ([twin.x, twin.buf] + ([twin.v] if kind == "lamb" else []))]
        for t, d in zip([twin.x, twin.buf] + ([twin.v] if kind == "lamb" else []),
                        [dev.x, dev.buf] + ([dev.v] if kind == "lamb" else [])):
            d.copy_(t)  # both start the step from the twin's fp32 state
        _step(dev, k)
        _step(twin, k)
        for sync in (dev, twin):
            post = [t.cpu().numpy() for t in ([sync.x, sync.buf] + ([sync.v] if kind == "lamb" else []))]
            trust = sync.trust_ratios().flip(0).numpy()
            for i, (o, n, ad) in enumerate(sync.lw_rows):
                sl = slice(o, o + n)
                L.check_tensor(kind, f"step {k} row {i}", (pre[0][sl], twin.g.numpy()[sl], *(a[sl] for a in pre[1:])),
                               tuple(a[sl] for a in post), trust[i], block, L.LR, 0.01, 1.0, ad)
    assert dev.trust_ratios().shape == (len(dev.params),)
    resumed = mk(device)
    resumed.x.copy_(dev.x)
    resumed.load_state_dict(dev.state_dict())
    _step(dev, 7)
    _step(resumed, 7)
    mine = [dev.x, dev.buf, dev.lw.trust] + ([dev.v, dev.lw.block] if kind == "lamb" else [])
    theirs = [resumed.x, resumed.buf, resumed.lw.trust] + ([resumed.v, resumed.lw.block] if kind == "lamb" else [])
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(mine, theirs))
