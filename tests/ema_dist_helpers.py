"""Rank body of the two-rank weight-EMA test (module-level so ``spawn`` can pickle it)."""
from __future__ import annotations

import os

import torch
import torch.distributed as dist


def ema_rank_body(rank, world, out_dir, kind, decay, steps):
    """Train a small MLP on rank-dependent data with an EMA attached; dump parameters and shadow."""
    from network_distributed_pytorch_amd import ops
    from network_distributed_pytorch_amd.parallel.comm import Communicator
    from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync

    dist.init_process_group("gloo", init_method="env://", rank=rank, world_size=world)
    torch.manual_seed(1000 + rank)  # different init per rank: the sync broadcasts
    model = torch.nn.Sequential(torch.nn.Linear(12, 16), torch.nn.Tanh(), torch.nn.Linear(16, 5))
    sync = build_grad_sync(kind, model, Communicator(), lr=0.05, momentum=0.9, rank=2)
    ema = ops.WeightEma([p.detach() for p in model.parameters()], decay)
    sync.attach_ema(ema)
    g = torch.Generator().manual_seed(7 + rank)
    for _ in range(steps):
        x = torch.randn(16, 12, generator=g) * (1.0 + 2.0 * rank)
        y = torch.randint(0, 5, (16,), generator=g)
        sync.zero_grad()
        torch.nn.functional.cross_entropy(model(x), y).backward()
        sync.step()
    torch.save({"params": [p.detach().clone() for p in model.parameters()],
                "shadow": [s.detach().clone() for s in ema.shadow], "block": ema.read()},
               os.path.join(out_dir, f"{kind}_rank{rank}.pt"))
    dist.destroy_process_group()
