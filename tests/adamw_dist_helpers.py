"""Rank body of the two-rank AdamW test (module-level so ``spawn`` can pickle it)."""
from __future__ import annotations

import os

import torch
import torch.distributed as dist

LR, WD, BETAS, EPS = 0.01, 0.1, (0.9, 0.99), 1e-8


def make_model():
    return torch.nn.Sequential(torch.nn.Linear(12, 16), torch.nn.Tanh(), torch.nn.Linear(16, 5))


def adamw_rank_body(rank, world, out_dir, steps, decay_1d):
    """Train a small MLP on rank-dependent data through the dense sync with AdamW; dump the initial
    (broadcast) parameters, every step's local gradients and the final parameters, moments, block."""
    from network_distributed_pytorch_amd.parallel.comm import Communicator
    from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync

    dist.init_process_group("gloo", init_method="env://", rank=rank, world_size=world)
    torch.manual_seed(1000 + rank)  # different init per rank: the sync broadcasts
    model = make_model()
    sync = build_grad_sync("dense", model, Communicator(), lr=LR, optimizer="adamw", betas=BETAS, eps=EPS,
                           decay_1d=decay_1d)
    sync.set_hyper(LR, WD)
    init = [p.detach().clone() for p in model.parameters()]
    g = torch.Generator().manual_seed(7 + rank)
    grads = []
    for _ in range(steps):
        x = torch.randn(16, 12, generator=g) * (1.0 + 2.0 * rank)
        y = torch.randint(0, 5, (16,), generator=g)
        sync.zero_grad()
        torch.nn.functional.cross_entropy(model(x), y).backward()
        grads.append([p.grad.detach().clone() for p in model.parameters()])
        sync.step()
    ddp = sync.ddp
    moments = []
    for p in model.parameters():
        o = ddp.offsets[id(p)]
        moments.append((ddp.buf[o: o + p.numel()].clone().view_as(p), ddp.v[o: o + p.numel()].clone().view_as(p)))
    torch.save({"init": init, "grads": grads, "params": [p.detach().clone() for p in model.parameters()],
                "moments": moments, "block": sync.adam_stats()},
               os.path.join(out_dir, f"adamw_rank{rank}.pt"))
    dist.destroy_process_group()
