"""Rank body of the two-rank gradient-clipping test (module-level so ``spawn`` can pickle it)."""
from __future__ import annotations

import os

import torch
import torch.distributed as dist


def clip_rank_body(rank, world, out_dir, kind, max_norm, steps):
    """Train a small MLP on rank-dependent data with a clip that bites; dump parameters and norms."""
    from network_distributed_pytorch_amd.parallel.comm import Communicator
    from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync

    dist.init_process_group("gloo", init_method="env://", rank=rank, world_size=world)
    torch.manual_seed(1000 + rank)  # different init per rank: the sync broadcasts
    model = torch.nn.Sequential(torch.nn.Linear(12, 16), torch.nn.Tanh(), torch.nn.Linear(16, 5))
    sync = build_grad_sync(kind, model, Communicator(), lr=0.05, momentum=0.9, rank=2, max_grad_norm=max_norm)
    g = torch.Generator().manual_seed(7 + rank)
    stats = []
    for _ in range(steps):
        x = torch.randn(16, 12, generator=g) * (1.0 + 2.0 * rank)  # rank 1's gradients are larger
        y = torch.randint(0, 5, (16,), generator=g)
        sync.zero_grad()
        torch.nn.functional.cross_entropy(model(x), y).backward()
        sync.step()
        stats.append(sync.clip_stats())
    torch.save({"params": [p.detach().clone() for p in model.parameters()], "stats": stats},
               os.path.join(out_dir, f"{kind}_rank{rank}.pt"))
    dist.destroy_process_group()
