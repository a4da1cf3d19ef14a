"""Shared by the PowerSGD + AdamW tests: the small MLP, per-step hyper-parameters and gradients, the
state of an optimiser as bits, and the rank body of the two-rank test (module-level so ``spawn`` can
pickle it)."""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.distributed as dist

RANK = 4
BETAS, EPS = (0.9, 0.99), 1e-8
HYPER = ((0.01, 0.1), (0.007, 0.0), (0.004, 0.25))  # (lr, wd) per step: both change, wd passes through 0


def make_model(seed=3):
    """weights [5, 7] (m % 4 != 0, r = 4) and [3, 5] (n < rank: r = 3), two biases"""
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3))


def batch(k, rank=0):
    g = torch.Generator().manual_seed(1000 * rank + 50 + k)
    return torch.randn(6, 7, generator=g) * (1.0 + rank), torch.randint(0, 3, (6,), generator=g)


def backward(sync, model, k, rank=0, device=None):
    sync.zero_grad()
    x, y = batch(k, rank)
    if device is not None:
        x, y = x.to(device), y.to(device)
    torch.nn.functional.cross_entropy(model(x), y).backward()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().copy()


def state_bits(opt):
    """every array of the optimiser's training state, as bits, plus the block"""
    return {"x": bits(opt.x), "m": bits(opt.m), "v": bits(opt._v), "e": bits(opt.e), "q": bits(opt.buf.q_warm),
            "block": opt.adam_stats()}


def same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], (k, a[k], b[k])


def fixed_grads(model, k, rank, same_mats):
    """seeded gradients set by hand: the <=1-D ones depend on the rank; the matrices' too unless
    ``same_mats``"""
    out = []
    for i, p in enumerate(model.parameters()):
        r = 0 if (same_mats and p.dim() > 1) else rank
        g = torch.Generator().manual_seed(7919 * r + 100 * k + i)
        out.append(torch.randn(p.shape, generator=g) * (1.0 + 2.0 * r))
    return out


def psgd_adam_rank_body(rank, world, out_dir, steps, decay_1d, same_mats):
    from network_distributed_pytorch_amd.parallel.comm import Communicator
    from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync

    dist.init_process_group("gloo", init_method="env://", rank=rank, world_size=world)
    model = make_model(seed=1000 + rank)  # different init per rank: the sync broadcasts
    sync = build_grad_sync("powersgd-adamw", model, Communicator(), lr=HYPER[0][0], rank=RANK, betas=BETAS, eps=EPS,
                           decay_1d=decay_1d)
    init = sync.x.clone()
    grads = []
    for k in range(steps):
        sync.set_hyper(*HYPER[k % len(HYPER)])
        sync.zero_grad()
        gs = fixed_grads(model, k, rank, same_mats)
        for p, g in zip(model.parameters(), gs):
            p.grad = g.clone()
        grads.append(gs)
        sync.step()
    torch.save({"init": init, "grads": grads, "x": sync.x.clone(), "m": sync.m.clone(), "v": sync._v.clone(),
                "e": sync.e.clone(), "q": sync.buf.q_warm.clone(), "block": sync.adam_stats()},
               os.path.join(out_dir, f"psgd_adam_rank{rank}.pt"))
    dist.destroy_process_group()
