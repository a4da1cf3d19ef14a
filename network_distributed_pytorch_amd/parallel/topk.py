"""Top-k gradient sparsification with error feedback as a :class:`GradSync` (``grad_sync="topk"``).

Every rank keeps the exact ``k`` largest-magnitude entries of ``m = g + e`` over the whole flat
gradient arena, feeds the rest back through the error memory ``e``, all-gathers the ``(idx, val)``
pairs and applies momentum SGD to the decompressed average (ops/topk.py has the rule; the momentum
sits behind the decompression, as in PowerSGD's Algorithm 2, so the two compressors compare).

* Arenas ``x`` / ``g`` / ``buf`` / ``e`` laid out like the dense arm's (reverse parameter order, each
  parameter padded to 16 elements, padding zero: a zero never beats a selected entry unless ``k``
  exceeds the non-zero entries, and then it decompresses to zero).  Parameters are re-pointed
  into ``x``; the native backwards write into ``g`` (ops/gradarena.py) and one :class:`SegPlan`
  flatten copies the gradients that did not land there.
* ``k = max(1, ceil(topk_ratio * P))`` with ``P`` the true parameter count, fixed at construction:
  every buffer and the collective have a static size, so the step can be captured.
* One step = [clip this rank's ``g``] + flatten + 5 select launches, ONE all-gather of ``int32[2k]``
  per rank (none at world size 1), 1 update launch, the EMA tail.  ``bytes_per_step = 8k``.
* No backward overlap: the global selection needs every gradient (``overlap=True`` raises, as for
  the clipped PowerSGD arm).
"""
from __future__ import annotations

from typing import List, Optional

import torch

from ..ops import SegPlan, capturing, gradarena, gradfinish
from ..ops.hyper import HyperState
from ..ops.topk import TopKCore, topk_count
from .comm import Communicator
from .ef_adam import EfAdam
from .sync import GradSync

__all__ = ["TopKSync"]


class TopKSync(EfAdam, HyperState, GradSync):
    _arm = "top-k arm"

    def __init__(self, model: torch.nn.Module, comm: Optional[Communicator] = None, lr: float = 1e-3,
                 momentum: float = 0.9, topk_ratio: float = 0.01, broadcast_params: bool = True,
                 overlap: Optional[bool] = None, weight_decay: float = 0.0, max_grad_norm: float = 0.0,
                 optimizer: str = "sgd", betas=(0.9, 0.999), eps: float = 1e-8, decay_1d: bool = True):
        assert weight_decay >= 0, "weight_decay >= 0"
        if overlap:
            raise ValueError("top-k: overlap=True is not available (the global selection needs every gradient "
                             "before its first launch)")
        self.model = model
        self.comm = comm if comm is not None else Communicator()
        self.momentum = float(momentum)
        self.topk_ratio = float(topk_ratio)
        self.params: List[torch.nn.Parameter] = [p for p in model.parameters() if p.requires_grad]
        self.device = self.params[0].device
        self._init_hyper(float(lr), float(weight_decay), block=self.device.type == "cuda",
                         on=self._init_optimizer(optimizer, betas, eps, decay_1d))
        offs, o = {}, 0
        for p in reversed(self.params):
            offs[id(p)] = o
            o += (p.numel() + 15) // 16 * 16
        self.numel, self.offsets = o, offs
        self.k = topk_count(sum(p.numel() for p in self.params), self.topk_ratio, o)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.x, self.g, self.buf, self.e = (torch.zeros(o, **f32) for _ in range(4))
        with torch.no_grad():
            for p in self.params:
                v = self.x[offs[id(p)]: offs[id(p)] + p.numel()].view_as(p)
                v.copy_(p.data)
                p.data = v
                p.grad = None
        if broadcast_params:
            self.comm.broadcast(self.x, src=0)
        if self.device.type == "cuda":
            for p in self.params:
                gradarena.register(p, self.g, offs[id(p)])
        self.world = self.comm.world_size if self.comm.active else 1
        self.core = TopKCore(self.device, o, self.k, self.world)
        self._alloc_adam(lambda: self.core.decay_runs([(offs[id(p)], self._decays(p)) for p in self.params]))
        self._seg = SegPlan([], self.device, capacity=len(self.params))
        self.step_count = 0
        self._init_clip(max_grad_norm, self.device, capacity=1, blocks=(o + 2047) // 2048)
        if self.clip is not None:
            self.clip.bind([self.g])

    @property
    def flat_weights(self) -> torch.Tensor:
        return self.x

    @property
    def bytes_per_step(self) -> int:
        return 8 * self.k

    @property
    def collectives_per_step(self) -> int:
        return 1 if self.comm.active else 0

    def collective_payloads(self):
        """Bytes this rank contributes to the step's one all-gather (link-model input)."""
        return [8 * self.k]

    def check_errors(self):
        self.comm.check()

    # -- the three phases --------------------------------------------------------------------------
    @torch.no_grad()
    def phase_select(self):
        gradfinish.flush()  # deferred conv grad-W sums / folds
        specs = []
        for p in self.params:
            o = self.offsets[id(p)]
            dst = self.g[o: o + p.numel()]
            if p.grad is None:  # unused parameter: zero gradient, in place
                p.grad = dst.view_as(p)
                p.grad.zero_()
            if p.grad.data_ptr() != dst.data_ptr():
                specs.append((p.grad.reshape(-1), dst, 1, 0, 1.0))
        self._seg.set(specs)
        self._seg.run()  # one flatten launch (only the gradients that did not land in the arena)
        if self.clip is not None:  # this rank's own gradient, before m = g + e
            self.clip.bind([self.g])
            self.clip.run(self.max_grad_norm)
        self.core.select(self.g, self.e)

    @torch.no_grad()
    def phase_gather(self):
        if self.comm.has_traffic:
            self.comm.all_gather_into(self.core.gathered, self.core.out)

    @torch.no_grad()
    def phase_update(self):
        self._update()
        self._after_update()  # the EMA reads the weights the update wrote: same stream, behind it
        self.count_step()

    def phases(self):
        return [(self.phase_select, False), (self.phase_gather, True), (self.phase_update, False)]

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            p.grad = None
        gradarena.release(self.params)

    def step(self) -> int:
        self.phase_select()
        self.phase_gather()
        self.phase_update()
        return 8 * self.bytes_per_step

    def count_step(self):
        if not capturing():
            self.step_count += 1

    # -- state ---------------------------------------------------------------------------------------
    def snapshot(self):
        return {"x": self.x.clone(), "buf": self.buf.clone(), "e": self.e.clone(), "step_count": self.step_count,
                **({"block": self.core.block.clone()} if self.core.block is not None else {}),
                **self._adam_snapshot(), **self._snapshot_extras()}

    def restore(self, snap):
        self.x.copy_(snap["x"])
        self.buf.copy_(snap["buf"])
        self.e.copy_(snap["e"])
        self.step_count = snap["step_count"]
        if self.core.block is not None:
            self.core.block.copy_(snap["block"])
        self._adam_restore(snap)
        self._restore_extras(snap)

    def state_dict(self):
        return {"error_memory": self.e.detach().cpu().clone(), **self._moments_state_dict(),
                "lr": self.lr, "momentum": self.momentum, "weight_decay": self.weight_decay, "k": self.k}

    def load_state_dict(self, sd):
        self._check_optimizer_state(sd)
        if int(sd["k"]) != self.k:
            raise ValueError(f"top-k arm: the checkpoint was written with k = {sd['k']}, this sync has k = {self.k}")
        self.e.copy_(sd["error_memory"])
        self._load_moments(sd)
        self.momentum = float(sd["momentum"])
        self._load_hyper(float(sd["lr"]), float(sd.get("weight_decay", 0.0)))
