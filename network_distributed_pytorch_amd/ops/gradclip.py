"""Global-norm gradient clipping on gfx950 (csrc/gradclip.hip): ``torch.nn.utils.clip_grad_norm_``
with ``error_if_nonfinite=False`` over any number of fp32 gradients in TWO launches, with a
deterministic fixed-order fp64 reduction and gradient-norm telemetry kept on the device.

The rule (identical on the device and in the torch twin that CPU tensors run), for tensors
``t_0 .. t_{k-1}``, ``max_norm`` > 0 (``inf``: measure, never scale) and ``div`` >= 1:

1. ``S = sum v^2`` over every element, each square formed and accumulated in fp64
   (``acc = fma((double)v, (double)v, acc)``): a tensor holding ``1e25`` has a finite norm.
2. ``norm = (float)(sqrt(S) / (double)div)``, rounded to fp32 once.
3. ``q = max_norm / (norm + 1e-6f)`` in fp32; ``coef = q if (q < 1 or q != q) else 1``.  A NaN
   norm gives a NaN coefficient, as ``torch.clamp`` does.
4. ``coef != 1``: every element becomes ``v * coef`` (one fp32 multiply).  ``coef == 1``: nothing
   is written; the tensors stay bitwise as they were, ``-0`` and NaN payloads included.
5. The block ``{float norm; float coef; uint32 clipped; uint32 steps}``: every run overwrites
   ``norm`` and ``coef``, does ``steps += 1`` and, when ``coef != 1``, ``clipped += 1``.

The device sums in the kernel's own fixed order (its header), the twin per tensor in list order
(``t.double().pow(2).sum()``): two fp64 sums in different orders can move the fp32-rounded norm by
one ulp, never more.  The device result is bitwise reproducible from run to run and under
hipGraph replay.  ``max_norm`` and ``div`` go to the kernel by value, so a captured graph freezes
them.
"""
from __future__ import annotations

from typing import Any, Dict, List, Sequence

import numpy as np
import torch

from . import SegPlan, StateBlock
from ._ext import ext

__all__ = ["GradClip", "clip_grad_norm_"]


def _check_args(max_norm: float, div: float):
    max_norm, div = float(max_norm), float(div)
    if not max_norm > 0.0:
        raise ValueError(f"gradient clipping: max_norm must be > 0 (inf: measure only), got {max_norm}")
    if not div >= 1.0:
        raise ValueError(f"gradient clipping: div must be >= 1, got {div}")
    return max_norm, div


def _twin(tensors: Sequence[torch.Tensor], max_norm: float, div: float):
    """Steps 1-4 of the rule in torch / numpy scalars; returns (norm, coef) as np.float32."""
    S = np.float64(0.0)
    for t in tensors:
        S = S + np.float64(t.detach().double().pow(2).sum().item())
    with np.errstate(all="ignore"):
        norm = np.float32(np.sqrt(S) / np.float64(np.float32(div)))
        q = np.float32(max_norm) / (norm + np.float32(1e-6))
    coef = q if (q < np.float32(1.0) or q != q) else np.float32(1.0)
    if coef != np.float32(1.0):
        for t in tensors:
            t.detach().mul_(float(coef))
    return norm, coef


class GradClip:
    """The clip of the module docstring over a re-targetable list of tensors.

    On a device it owns the :class:`SegPlan` table (``capacity`` entries), the fp64 block partials
    (``blocks`` of 2048 elements, grown by an eager :meth:`bind` only), the arrival ticket and
    the 16-byte ``clip`` block; everything a captured step needs exists after construction plus
    one eager :meth:`bind`, or at construction when ``capacity`` / ``blocks`` cover the list.  On
    a CPU device the same class runs the torch twin.
    """

    def __init__(self, device, capacity: int = 0, blocks: int = 0):
        self.device = torch.device(device)
        self.tensors: List[torch.Tensor] = []
        self._retired: list = []  # outgrown partials: a captured graph may still hold the address
        self.state = StateBlock(self.device, ("norm", "coef", "clipped", "steps"), (0.0, 1.0, 0, 0))
        self.clip = self.state.dev  # the kernels' argument (None on CPU: the twin keeps a dict)
        self._empty = True  # the last run had nothing to reduce: norm 0, coef 1
        if self.device.type == "cuda":
            assert not torch.cuda.is_current_stream_capturing(), "GradClip is built before capture"
            self.plan = SegPlan((), self.device, capacity=max(int(capacity), 1))
            self.partial = torch.empty(max(int(blocks), 1), dtype=torch.float64, device=self.device)
            # the two-level arrival tickets of the table's workgroups: zero, re-armed by every launch
            self.ctr = torch.zeros(ext().arrive_ctr_words(self.partial.numel()), dtype=torch.int32,
                                   device=self.device)

    def bind(self, tensors: Sequence[torch.Tensor]) -> None:
        """Re-target the table at ``tensors`` (uploaded only when an address changed; inside a
        capture through :func:`ops.upload`, and never growing a buffer there)."""
        tensors = list(tensors)
        if self.device.type == "cuda":
            for t in tensors:
                if not (t.is_cuda and t.device == self.device):
                    raise ValueError(f"GradClip on {self.device}: tensor on {t.device}")
                if t.dtype != torch.float32 or not t.is_contiguous():
                    raise ValueError("GradClip: device tensors must be contiguous float32 "
                                     f"(got {t.dtype}, contiguous={t.is_contiguous()})")
            flat = [t.detach().reshape(-1) for t in tensors]
            self.plan.set([(f, f, 1, 0, 1.0) for f in flat])
            blocks = self.plan.n_blocks
            if blocks > self.partial.numel():
                assert not torch.cuda.is_current_stream_capturing(), "GradClip must be sized before graph capture"
                self._retired += [self.partial, self.ctr]
                self.partial = torch.empty(blocks, dtype=torch.float64, device=self.device)
                self.ctr = torch.zeros(ext().arrive_ctr_words(blocks), dtype=torch.int32, device=self.device)
        self.tensors = tensors

    def run(self, max_norm: float, div: float = 1.0) -> None:
        max_norm, div = _check_args(max_norm, div)
        if self.device.type == "cuda":
            X = ext()
            self._empty = not self.plan.launch(X.grad_sqnorm, self.partial, self.ctr, self.clip, max_norm, div)
            if not self._empty:
                self.plan.launch(X.grad_scale, self.clip)
            return
        self._empty = not any(t.numel() for t in self.tensors)
        if self._empty:
            return
        norm, coef = _twin(self.tensors, max_norm, div)
        st = self.state.read()
        self.state.write({"norm": float(norm), "coef": float(coef), "steps": st["steps"] + 1,
                          "clipped": st["clipped"] + int(coef != np.float32(1.0))})

    def snapshot(self):
        """The block's contents, for :meth:`restore` (a graph warm-up leaves no trace in the counters)."""
        return self.state.snapshot()

    def restore(self, snap) -> None:
        self.state.restore(snap)

    def norm_tensor(self) -> torch.Tensor:
        """The fp32 norm of the last run as a 0-dim tensor on the device (no host sync)."""
        if self._empty:
            return torch.zeros((), dtype=torch.float32, device=self.device)
        if self.device.type == "cuda":
            return self.clip[0:1].view(torch.float32).clone().reshape(())
        return torch.tensor(self.state.read()["norm"], dtype=torch.float32)

    def read(self) -> Dict[str, Any]:
        """``{"norm", "coef", "clipped", "steps"}`` of the block: a host sync on a device."""
        out = self.state.read()
        if self._empty:
            out["norm"], out["coef"] = 0.0, 1.0
        return out


def clip_grad_norm_(tensors: Sequence[torch.Tensor], max_norm: float, div: float = 1.0) -> torch.Tensor:
    """One-shot :class:`GradClip` over ``tensors`` (scaled in place); returns the fp32 norm."""
    tensors = [tensors] if isinstance(tensors, torch.Tensor) else list(tensors)
    device = tensors[0].device if tensors else torch.device("cpu")
    blocks = 0
    if device.type == "cuda":  # size the partials once; the twin that CPU tensors run has none
        per = ext().SEG_BLOCK_ELEMS
        blocks = sum((t.numel() + per - 1) // per for t in tensors)
    clip = GradClip(device, capacity=len(tensors), blocks=blocks)
    clip.bind(tensors)
    clip.run(max_norm, div)
    return clip.norm_tensor()
