"""AdamW in the flat-arena compressors: what :class:`TopKSync`, :class:`SignSync` and :class:`QuantSync`
share when they are built with ``optimizer="adamw"`` (``grad_sync="topk-adamw"``, ``"signsgd-adamw"``,
``"quant-adamw"``).

Everything up to the decompressed average ``o`` is the arm's own rule, launches and wire; behind it the
update launch runs the AdamW element rule of ops/adamw.py (``g := o``, ``div = 1``) in the place of
momentum SGD.  The momentum arena ``buf`` holds the first moment, a new arena ``v`` of the same layout
the second; the 16-byte block ``{b1pow, b2pow, steps}`` and the launch's tickets are an
:class:`ops.adamw.AdamState`, and the per-tensor decay flags (``decay_1d=False`` exempts tensors of at
most one dimension) are uploaded once.  All of it exists after construction, before any capture; the
update launch always reads ``lr`` / ``weight_decay`` from the hyper block; ``momentum`` is ignored.
"""
from __future__ import annotations

from typing import Any, Callable, Dict, Optional

import torch

from ..ops.adamw import AdamState, check_adam_args

__all__ = ["EfAdam"]


class EfAdam:
    optimizer = "sgd"
    adam: Optional[AdamState] = None

    def _init_optimizer(self, optimizer: str, betas, eps, decay_1d) -> Optional[bool]:
        """Checks and keeps the optimiser choice; returns ``_init_hyper``'s ``on`` (the AdamW launch
        has no by-value weight decay: it reads the block from the start)."""
        if optimizer not in ("sgd", "adamw"):
            raise ValueError(f"{self._arm}: unknown optimizer {optimizer!r} (sgd, adamw)")
        self.optimizer = optimizer
        if optimizer != "adamw":
            return None
        self.beta1, self.beta2, self.eps = check_adam_args(betas, eps)
        self.decay_1d = bool(decay_1d)
        return True

    def _decays(self, p: torch.Tensor) -> bool:
        return self.decay_1d or p.dim() > 1

    def _alloc_adam(self, decays: Callable[[], torch.Tensor]) -> None:
        """Second-moment arena, block, tickets and the decay flags ``decays()`` (the core's layout)."""
        if self.optimizer == "adamw":
            self.v = torch.zeros_like(self.buf)
            self.adam = AdamState(self.device, self.core.adam_grid)
            self.decays = decays()

    def _update(self) -> None:
        """The arm's one update launch (or twin) over the gathered buffers."""
        hy = self._hyper_arg()
        if self.adam is None:
            self.core.update(self.x, self.buf, self.core.gathered, self.lr, self.momentum, self.weight_decay, hy)
        else:
            self.core.update_adam(self.x, self.buf, self.v, self.core.gathered, self.lr, self.weight_decay, self.beta1,
                                  self.beta2, self.eps, self.adam, self.decays, hy)

    def adam_stats(self) -> Optional[Dict[str, Any]]:
        """``{"b1pow", "b2pow", "steps"}`` of the AdamW block (a host sync), or None with SGD."""
        return self.adam.read() if self.adam is not None else None

    def _adam_snapshot(self) -> Dict[str, Any]:
        return {"v": self.v.clone(), "adam": self.adam.snapshot()} if self.adam is not None else {}

    def _adam_restore(self, snap) -> None:
        if self.adam is not None:
            self.v.copy_(snap["v"])
            self.adam.restore(snap["adam"])

    def _moments_state_dict(self) -> Dict[str, Any]:
        """The optimiser's entries of ``state_dict()``: the momentum buffer, or the moments and block."""
        if self.adam is None:
            return {"momentum_buffer": self.buf.detach().cpu().clone()}
        st = self.adam.read()
        return {"optimizer": "adamw", "exp_avg": self.buf.detach().cpu().clone(),
                "exp_avg_sq": self.v.detach().cpu().clone(), "b1pow": st["b1pow"], "b2pow": st["b2pow"],
                "steps": st["steps"], "betas": (self.beta1, self.beta2), "eps": self.eps, "decay_1d": self.decay_1d}

    def _check_optimizer_state(self, sd) -> None:
        theirs = sd.get("optimizer", "sgd")  # a checkpoint without "optimizer" is an SGD checkpoint
        if theirs != self.optimizer:
            raise ValueError(f"{self._arm}: the checkpoint holds {theirs} optimizer state, this sync runs "
                             f"{self.optimizer}; they cannot be loaded into each other")

    def _load_moments(self, sd) -> None:
        if self.adam is None:
            self.buf.copy_(sd["momentum_buffer"])
            return
        if bool(sd["decay_1d"]) != self.decay_1d:
            raise ValueError(f"{self._arm}: the checkpoint was written with decay_1d = {sd['decay_1d']}, this sync "
                             f"has decay_1d = {self.decay_1d} (the decay flags are uploaded at construction)")
        self.buf.copy_(sd["exp_avg"])
        self.v.copy_(sd["exp_avg_sq"])
        self.adam.write(sd)  # betas / eps stay this sync's: a captured step holds them by value
