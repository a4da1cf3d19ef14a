"""``build_grad_sync(kind, model, comm, ...)``: the gradient-synchronisation strategies, each a
:class:`GradSync` (parallel/sync.py: the interface, and what every strategy has in common).

======================  =====================================================================
``powersgd``            :class:`PowerSGDSync`: the fused native engine (parallel/powersgd.py)
``powersgd-adamw``      :class:`PowerSGDSync` with ``optimizer="adamw"``: the same engine, AdamW in its update pass
``powersgd-ref``        :class:`ReferencePowerSGDLoop`, the reducer's torch path
``powersgd-api``        :class:`ReferencePowerSGDLoop`, the native reducer behind the reference API
``dense``               :class:`_DenseSync`: bucketed, backward-overlapped all-reduce (parallel/ddp.py)
``dense-ref``           :class:`ReferenceDenseLoop`: blocking per-parameter all-reduce + torch optimiser
``local-sgd-nesterov``  :class:`LocalOptimizer`, no communication
``local-adamw``         :class:`LocalOptimizer`, no communication
======================  =====================================================================
"""
from __future__ import annotations

from typing import Optional

import torch

from ..ops.adamw import FusedAdamW, check_adam_args
from .comm import Communicator
from .ddp import BucketedDataParallel, average_gradients
from .powersgd import PowerSGDOptimizer, PowerSGDReducer, powersgd_bytes_per_step
from .sync import GradSync

__all__ = ["build_grad_sync", "ReferencePowerSGDLoop", "ReferenceDenseLoop", "PowerSGDSync", "ADAMW_SYNCS"]

ADAMW_SYNCS = ("dense", "dense-ref", "powersgd-ref", "powersgd-api")  # the arms that take optimizer="adamw"


class PowerSGDSync(PowerSGDOptimizer):
    def __init__(self, model, comm, lr, momentum, rank, seed=714, **kw):
        super().__init__(model.parameters(), lr=lr, momentum=momentum, rank=rank, random_seed=seed, comm=comm, **kw)
        self.bytes_per_step = powersgd_bytes_per_step(list(model.parameters()), rank)["total"]

    @property
    def opt(self):
        """Compatibility name from when this class wrapped the optimiser: the object itself."""
        return self


class ReferencePowerSGDLoop(GradSync):
    """Algorithm 2 exactly as the reference loop writes it (ddp_init.py:130-178)."""

    def __init__(self, model, comm, lr, momentum, rank, seed=714, native_reducer=False, max_grad_norm=0.0,
                 optimizer="sgd", betas=(0.9, 0.999), eps=1e-8, decay_1d=True):
        self.model = model
        self.params = list(model.parameters())
        # optimizer="adamw": ops.FusedAdamW over the decompressed, averaged gradients the reducer
        # wrote, in the place of the momentum + SGD lines; error memory and wire untouched
        self.adam = None
        if optimizer == "adamw":
            self.adam = FusedAdamW(self.params, lr, betas=betas, eps=eps,
                                   decay_mask=[decay_1d or p.dim() > 1 for p in self.params])
        elif optimizer != "sgd":
            raise ValueError(f"unknown optimizer {optimizer!r} (sgd, adamw)")
        self._init_clip(max_grad_norm, self.params[0].device)
        self.lr, self.lam, self.weight_decay = lr, momentum, 0.0
        self.reducer = PowerSGDReducer(seed, self.params[0].device, 0, True, rank=rank, comm=comm)
        self.native_reducer = native_reducer
        self.memories = [torch.zeros_like(p) for p in self.params]
        self.send_buffers = [torch.zeros_like(p) for p in self.params]
        self.momenta = [torch.empty_like(p) for p in self.params]
        self.first = True
        self.bits = 0
        b = powersgd_bytes_per_step(self.params, rank)
        self.bytes_per_step = b["total"]
        self._payloads = [b["p"], b["rank1"], b["q"]]  # reducer.py:126, :132, :145
        self.collectives_per_step = 3 if comm.active else 0

    def collective_payloads(self):
        return list(self._payloads)

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    def set_hyper(self, lr, weight_decay=None):
        self.lr = float(lr)
        if weight_decay is not None:
            self.weight_decay = float(weight_decay)
        if self.adam is not None:
            self.adam.set_hyper(lr, weight_decay)

    def adam_stats(self):
        return self.adam.read() if self.adam is not None else None

    @torch.no_grad()
    def step(self):
        grads = [p.grad for p in self.params]
        self._clip_grads(grads)  # this rank's own gradient, before s = g + e
        for g, e, s in zip(grads, self.memories, self.send_buffers):
            s.data[:] = g + e
        if self.native_reducer:
            self.bits += self.reducer.reduce(self.send_buffers, grads, self.memories)
        else:
            self.bits += self.reducer.reduce_torch(self.send_buffers, grads, self.memories)
        if self.adam is not None:  # decoupled decay, moments and the step in one launch (twin on CPU)
            self.adam.bind(grads)
            self.adam.step()
            self._after_update()
            return self.bytes_per_step * 8
        if self.weight_decay != 0.0:  # L2 on the decompressed gradient: never in the memory or on the wire
            for p, g in zip(self.params, grads):
                g.add_(p, alpha=self.weight_decay)
        for g, m in zip(grads, self.momenta):
            if self.first:
                m.data = g.clone().detach()
            else:
                m.mul_(self.lam).add_(g)
            g.data[:] += m
        self.first = False
        for p, g in zip(self.params, grads):
            p.data.add_(g, alpha=-self.lr)
        self._after_update()
        return self.bytes_per_step * 8


class ReferenceDenseLoop(GradSync):
    def __init__(self, model, comm, lr, momentum, max_grad_norm=0.0, optimizer="sgd", betas=(0.9, 0.999), eps=1e-8,
                 decay_1d=True):
        self.model = model
        self.comm = comm
        self._init_clip(max_grad_norm, next(model.parameters()).device)
        self.optimizer = optimizer
        if optimizer == "adamw":
            # torch.optim.AdamW with two param groups: the reference-semantics comparison arm
            b1, b2, eps = check_adam_args(betas, eps)
            ps = list(model.parameters())
            groups = [{"params": [p for p in ps if decay_1d or p.dim() > 1], "decays": True},
                      {"params": [p for p in ps if not (decay_1d or p.dim() > 1)], "decays": False}]
            # capturable on a device: torch refuses to capture AdamW's host-side step count otherwise
            self.opt = torch.optim.AdamW([g for g in groups if g["params"]], lr=lr, betas=(b1, b2), eps=eps,
                                         weight_decay=0.0, capturable=ps[0].is_cuda)
        elif optimizer == "sgd":
            self.opt = torch.optim.SGD(model.parameters(), lr=lr, momentum=momentum)
        else:
            raise ValueError(f"unknown optimizer {optimizer!r} (sgd, adamw)")
        self.bytes_per_step = 4 * sum(p.numel() for p in model.parameters())
        self._payloads = [4 * p.numel() for p in model.parameters()]  # ddp_init.py:61, one per param
        self.collectives_per_step = len(list(model.parameters())) if comm.active else 0

    def collective_payloads(self):
        return list(self._payloads)

    def zero_grad(self):
        self.opt.zero_grad()

    def set_hyper(self, lr, weight_decay=None):
        _set_param_groups(self.opt, lr, weight_decay)

    def adam_stats(self):
        if self.optimizer != "adamw":
            return None
        steps = [int(s["step"]) for s in self.opt.state.values() if "step" in s]
        return {"steps": max(steps) if steps else 0}

    def step(self):
        bits = average_gradients(self.model, self.comm)
        self._clip_grads([p.grad for p in self.model.parameters()])
        self.opt.step()
        self._after_update()
        return bits


class _DenseSync(BucketedDataParallel):
    def __init__(self, model, comm, lr, momentum, bucket_mb, overlap=None, max_grad_norm=0.0, **adam):
        # adam: optimizer / betas / eps / decay_1d, only when the optimiser is not SGD
        super().__init__(model, comm, lr=lr, momentum=momentum, bucket_mb=bucket_mb, overlap=overlap,
                         max_grad_norm=max_grad_norm, **adam)

    @property
    def ddp(self):
        """Compatibility name from when this class wrapped the data-parallel engine: the object itself."""
        return self


def _set_param_groups(opt: torch.optim.Optimizer, lr, weight_decay):
    for group in opt.param_groups:
        group["lr"] = float(lr)
        if weight_decay is not None and group.get("decays", True):  # AdamW's exempt group stays at 0
            group["weight_decay"] = float(weight_decay)


def build_grad_sync(kind: str, model: torch.nn.Module, comm: Optional[Communicator] = None, lr: float = 1e-3,
                    momentum: float = 0.9, rank: int = 4, bucket_mb: Optional[float] = None, seed: int = 714,
                    max_grad_norm: float = 0.0, optimizer: str = "sgd", betas=(0.9, 0.999), eps: float = 1e-8,
                    decay_1d: bool = True, **kw):
    comm = comm if comm is not None else Communicator()
    clip = {"max_grad_norm": max_grad_norm} if max_grad_norm else {}  # off: every constructor call as before
    adam = {}  # optimizer="sgd": every constructor call as before
    if kind == "powersgd-adamw":
        # the kind is the optimiser choice (as local-adamw): optimizer "sgd" here means "unspecified"
        if optimizer not in ("sgd", "adamw"):
            raise ValueError(f"unknown optimizer {optimizer!r} (sgd, adamw)")
        b1, b2, eps = check_adam_args(betas, eps)
        return PowerSGDSync(model, comm, lr, momentum, rank, seed=seed, optimizer="adamw", betas=(b1, b2),
                            eps_adam=eps, decay_1d=bool(decay_1d), **clip, **kw)
    if optimizer != "sgd":
        if optimizer != "adamw":
            raise ValueError(f"unknown optimizer {optimizer!r} (sgd, adamw)")
        if kind not in ADAMW_SYNCS:
            raise ValueError(f"grad sync {kind!r} has no AdamW: the fused PowerSGD update kernels decompress, feed "
                             f"back and step in one register-pinned pass (an Adam variant of them is future work) and "
                             f"the local optimisers are fixed recipes; use one of {', '.join(ADAMW_SYNCS)}")
        b1, b2, eps = check_adam_args(betas, eps)
        adam = {"optimizer": "adamw", "betas": (b1, b2), "eps": eps, "decay_1d": bool(decay_1d)}
    if kind == "powersgd":
        return PowerSGDSync(model, comm, lr, momentum, rank, seed=seed, **clip, **kw)
    if kind == "powersgd-ref":
        return ReferencePowerSGDLoop(model, comm, lr, momentum, rank, seed=seed, **clip, **adam)
    if kind == "powersgd-api":
        return ReferencePowerSGDLoop(model, comm, lr, momentum, rank, seed=seed, native_reducer=True, **clip, **adam)
    if kind == "dense":
        return _DenseSync(model, comm, lr, momentum, bucket_mb, overlap=kw.get("overlap"), **clip, **adam)
    if kind == "dense-ref":
        return ReferenceDenseLoop(model, comm, lr, momentum, **clip, **adam)
    if kind in ("local-sgd-nesterov", "local-adamw"):
        return LocalOptimizer(model, kind, lr, momentum, **clip)
    raise ValueError(f"unknown grad sync {kind!r}")


class LocalOptimizer(GradSync):
    """Single-GPU baselines, no communication (reference C17):
    ``local-sgd-nesterov`` = SGD(lr, momentum=0.9, nesterov=True)
    (ddp_powersgd_distillBERT_IMDb/IMDb_distillBERT_example.py:57);
    ``local-adamw`` = AdamW(lr) (IMDb_dataset_distributer.py:55)."""

    def __init__(self, model, kind, lr, momentum, max_grad_norm=0.0):
        self.model = model
        self._init_clip(max_grad_norm, next(model.parameters()).device)
        if kind == "local-adamw":
            self.opt = torch.optim.AdamW(model.parameters(), lr=lr)
        else:
            self.opt = torch.optim.SGD(model.parameters(), lr=lr, momentum=momentum, nesterov=True)

    def zero_grad(self):
        self.opt.zero_grad()

    def set_hyper(self, lr, weight_decay=None):
        _set_param_groups(self.opt, lr, weight_decay)

    def step(self):
        self._clip_grads([p.grad for p in self.model.parameters()])
        self.opt.step()
        self._after_update()
        return 0

    def state_dict(self):
        return self.opt.state_dict()

    def load_state_dict(self, sd):
        self.opt.load_state_dict(sd)
