"""Block-quantised gradient compression with error feedback as a :class:`GradSync` (``grad_sync="quant"``).

Every rank sends a ``quant_bits``-bit fixed-point code per coordinate of ``m = g + e`` (2, 4 or 8 bits;
ternary at 2) and one fp32 scale per block of 2048 elements of a tensor (the block's absmax over the
largest code), feeds ``m - c`` back through the error memory ``e``, all-gathers the rows and applies
momentum SGD to the decoded average (ops/quant.py has the rule; QSGD of Alistarh et al. 2017 and
TernGrad of Wen et al. 2017, here with deterministic rounding and error feedback).

Arenas, block table, phases, clipping, EMA tail and state are :class:`SignSync`'s; only the core
differs.  One step = [clip] + flatten + 1 pack launch, ONE all-gather of ``int32[row_words]`` per rank
(none at world size 1), 1 update launch, the EMA tail.  ``bytes_per_step = 4 * row_words``, about
``32 / quant_bits`` times below dense.  No backward overlap, as in the scaled-sign arm;
``optimizer="adamw"`` (``adam``: ``optimizer`` / ``betas`` / ``eps`` / ``decay_1d``) as there too
(parallel/ef_adam.py).

``quant_rotate="hadamard"`` quantises every full block behind a randomized Hadamard rotation (ops/quant.py
has the rule): the same wire, launches and bytes; the error memory of those blocks then lives in the
rotated domain, so a checkpoint loads only into a sync with the same ``quant_rotate`` and
``quant_rotate_seed``.  Every rank must be built with the same seed (it fixes the signs).
"""
from __future__ import annotations

from typing import Optional

import torch

from ..ops.quant import QUANT_BITS, QUANT_ROTATIONS, QuantCore
from .comm import Communicator
from .signsgd import SignSync

__all__ = ["QuantSync"]


class QuantSync(SignSync):
    _arm = "quant arm"

    def __init__(self, model: torch.nn.Module, comm: Optional[Communicator] = None, lr: float = 1e-3,
                 momentum: float = 0.9, broadcast_params: bool = True, overlap: Optional[bool] = None,
                 weight_decay: float = 0.0, max_grad_norm: float = 0.0, quant_bits: int = 4,
                 quant_rotate: str = "none", quant_rotate_seed: int = 0, **adam):
        if quant_bits not in QUANT_BITS:
            raise ValueError(f"quant: quant_bits must be one of {QUANT_BITS}, got {quant_bits!r}")
        if quant_rotate not in QUANT_ROTATIONS:
            raise ValueError(f"quant: quant_rotate must be one of {QUANT_ROTATIONS}, got {quant_rotate!r}")
        if overlap:
            raise ValueError("quant: overlap=True is not available (per-tensor packing during the backward is out "
                             "of scope here, as in the signsgd arm)")
        self.bits, self.rotate, self.rotate_seed = int(quant_bits), quant_rotate, int(quant_rotate_seed)
        super().__init__(model, comm, lr=lr, momentum=momentum, broadcast_params=broadcast_params,
                         weight_decay=weight_decay, max_grad_norm=max_grad_norm, **adam)

    def _build_core(self, segments, n):
        return QuantCore(self.device, segments, n, self.world, self.bits, self.rotate, self.rotate_seed)

    def state_dict(self):
        return {**super().state_dict(), "bits": self.bits, "rotate": self.rotate, "rotate_seed": self.rotate_seed}

    def load_state_dict(self, sd):
        if int(sd["bits"]) != self.bits:
            raise ValueError(f"{self._arm}: the checkpoint was written with bits = {sd['bits']}, this sync has "
                             f"bits = {self.bits} (the error memory holds the residual of that code)")
        theirs = (sd.get("rotate", "none"), int(sd.get("rotate_seed", 0)))  # no keys: written before the rotation
        if theirs != (self.rotate, self.rotate_seed) and (theirs[0], self.rotate) != ("none", "none"):
            raise ValueError(f"{self._arm}: the checkpoint was written with rotate = {theirs[0]!r}, rotate_seed = "
                             f"{theirs[1]}, this sync has rotate = {self.rotate!r}, rotate_seed = {self.rotate_seed} "
                             f"(the error memory of a full block is in that rotation's domain)")
        super().load_state_dict(sd)
