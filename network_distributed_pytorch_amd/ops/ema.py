"""Exponential moving average of the weights on gfx950 (csrc/ema.hip): what
``torch.optim.swa_utils.AveragedModel`` with ``get_ema_multi_avg_fn`` or timm's ``ModelEmaV2``
keep, over any number of fp32 tensors in ONE launch whose step-dependent decay lives on the
device, so a captured step serves every step.

The rule (bitwise identical on the device and in the torch twin that CPU tensors run), for live
tensors ``x_i``, shadows ``s_i``, ``0 < decay < 1`` and ``warmup`` (both frozen into a captured
graph) and the block ``{float decay; float weight; uint32 updates; uint32 pad}``:

1. ``n = block.updates``, the number of runs before this one.
2. ``d = min(decay, (n + 1) / (n + 10))`` with warm-up (the TF / timm one: the first update moves
   the shadow 90 % of the way), ``d = decay`` without; all fp32, IEEE division, ``(float)n``
   rounded to nearest.  ``w = 1 - d``.
3. Every element: ``t = x - s``, ``u = w * t``, ``s' = s + u``: three single, correctly rounded
   fp32 operations, never a fused ``fma(w, t, s)``.  So ``x == s`` keeps the shadow, a shared
   ``-0`` becomes ``+0`` and ``x = s = inf`` gives NaN.
4. Once per run the block gets ``decay = d``, ``weight = w``, ``updates = n + 1``.

The shadow starts as a copy of the live tensors with ``updates = 0``.
"""
from __future__ import annotations

from typing import Any, Dict, List, Sequence

import numpy as np
import torch

from . import SegPlan, StateBlock
from ._ext import ext

__all__ = ["WeightEma", "ema_decay_at"]


def _check_decay(decay: float) -> float:
    decay = float(decay)
    if not (np.float32(0.0) < np.float32(decay) < np.float32(1.0)):
        raise ValueError(f"weight EMA: decay must be in (0, 1) as fp32, got {decay}")
    return decay


def ema_decay_at(decay: float, n: int, warmup: bool = True):
    """``(d, w)`` of the run that follows ``n`` earlier ones, as ``numpy.float32``: the Python
    twin of the kernel's schedule (step 2 of the rule)."""
    d = np.float32(decay)
    if warmup:
        fn = np.float32(int(n))
        num = fn + np.float32(1.0)
        den = fn + np.float32(10.0)
        r = num / den
        d = min(d, r)
    w = np.float32(1.0) - d
    return np.float32(d), np.float32(w)


class WeightEma:
    """The EMA of the module docstring over ``tensors`` (the live weights, updated in place by the
    optimiser; never re-targeted).

    Owns one flat fp32 shadow arena in which every shadow sits at its live tensor's offset from
    a 16-byte boundary (an aligned parameter keeps the float4 path), ``shadow`` (views shaped
    like ``tensors``), and on a device the :class:`SegPlan` table (live tensors that are adjacent
    in memory share one entry), the two-level arrival tickets and the 16-byte block.  Everything
    exists after construction, which is eager; :meth:`update` and :meth:`swap` are one launch
    each and capture-safe.  On a CPU device the same class runs the torch twin.
    """

    def __init__(self, tensors: Sequence[torch.Tensor], decay: float, warmup: bool = True):
        self.decay = _check_decay(decay)
        self.warmup = bool(warmup)
        self.tensors: List[torch.Tensor] = [t.detach() for t in tensors]
        if not self.tensors:
            raise ValueError("weight EMA: no tensors")
        self.device = self.tensors[0].device
        cuda = self.device.type == "cuda"
        if cuda:
            assert not torch.cuda.is_current_stream_capturing(), "WeightEma is built before capture"
        for t in self.tensors:
            if t.device != self.device:
                raise ValueError(f"WeightEma on {self.device}: tensor on {t.device}")
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("WeightEma: tensors must be contiguous float32 "
                                 f"(got {t.dtype}, contiguous={t.is_contiguous()})")
        # runs of tensors adjacent in one storage: [first index, element count, address, storage]
        runs: List[list] = []
        for i, t in enumerate(self.tensors):
            st = t.untyped_storage().data_ptr()
            if (runs and t.numel() and runs[-1][1] and runs[-1][3] == st
                    and runs[-1][2] + 4 * runs[-1][1] == t.data_ptr()):
                runs[-1][1] += t.numel()
            else:
                runs.append([i, t.numel(), t.data_ptr(), st])
        # arena offsets (floats): a run starts as far past a 16-byte boundary as its live memory
        offs, total = [], 0
        for _, n, addr, _ in runs:
            total = (total + 3) // 4 * 4 + (addr % 16) // 4
            offs.append(total)
            total += n
        self.arena = torch.zeros(max(total, 1), dtype=torch.float32, device=self.device)
        assert self.arena.data_ptr() % 16 == 0
        self.shadow: List[torch.Tensor] = []
        for r, run in enumerate(runs):
            o = offs[r]
            end = runs[r + 1][0] if r + 1 < len(runs) else len(self.tensors)
            for t in self.tensors[run[0]: end]:
                self.shadow.append(self.arena[o: o + t.numel()].view(t.shape))
                o += t.numel()
        with torch.no_grad():
            for s, t in zip(self.shadow, self.tensors):
                s.copy_(t)
        self.state = StateBlock(self.device, ("decay", "weight", "updates"), (0.0, 0.0, 0))
        self.block = self.state.dev  # the kernels' argument (None on CPU: the twin keeps a dict)
        if cuda:
            specs = []
            for r, (i0, n, _, _) in enumerate(runs):
                if n == 0:
                    continue
                first = self.tensors[i0]
                live = first.reshape(-1) if n == first.numel() else torch.as_strided(first, (n,), (1,))
                specs.append((live, self.arena[offs[r]: offs[r] + n], 1, 0, 1.0))
            self.plan = SegPlan(specs, self.device)
            self.ctr = torch.zeros(ext().arrive_ctr_words(self.plan.n_blocks), dtype=torch.int32, device=self.device)

    # ---- the rule ---------------------------------------------------------------------------
    def update(self) -> None:
        """One run of the rule: one launch on a device (current stream), the twin on CPU."""
        if self.device.type == "cuda":
            if not self.plan.launch(ext().ema_update, self.ctr, self.block, self.decay, self.warmup):
                raise RuntimeError("WeightEma.update: empty table")
            return
        n = self.state.read()["updates"]
        d, w = ema_decay_at(self.decay, n, self.warmup)
        with torch.no_grad():
            for s, x in zip(self.shadow, self.tensors):
                t = torch.sub(x, s)
                u = torch.mul(t, float(w))
                s.copy_(torch.add(s, u))
        self.state.write({"decay": float(d), "weight": float(w), "updates": n + 1})

    def swap(self) -> None:
        """Exchange live tensors and shadows bitwise (twice: the identity)."""
        if self.device.type == "cuda":
            self.plan.launch(ext().ema_swap)
            return
        with torch.no_grad():
            for s, x in zip(self.shadow, self.tensors):
                si, xi = s.view(torch.int32), x.view(torch.int32)  # as words: NaN payloads survive
                tmp = si.clone()
                si.copy_(xi)
                xi.copy_(tmp)

    # ---- state ------------------------------------------------------------------------------
    def read(self) -> Dict[str, Any]:
        """``{"decay", "weight", "updates"}`` of the block: a host sync on a device."""
        return self.state.read()

    def reset(self) -> None:
        """The state after construction: the shadow a copy of the live tensors, ``updates = 0``."""
        with torch.no_grad():
            for s, t in zip(self.shadow, self.tensors):
                s.copy_(t)
        self.state.write({"decay": 0.0, "weight": 0.0, "updates": 0})

    def snapshot(self):
        """Shadow and block, for :meth:`restore` (a graph warm-up leaves no trace)."""
        return self.arena.clone(), self.state.snapshot()

    def restore(self, snap) -> None:
        arena, blk = snap
        self.arena.copy_(arena)
        self.state.restore(blk)

    def state_dict(self, names: Sequence[str]) -> Dict[str, Any]:
        """``{"shadow": {name: CPU tensor}, "updates", "decay", "weight"}``; ``names`` are the
        model's ``state_dict`` names of ``tensors``, in order."""
        names = list(names)
        if len(names) != len(self.shadow):
            raise ValueError(f"WeightEma.state_dict: {len(names)} names for {len(self.shadow)} tensors")
        st = self.read()
        return {"shadow": {k: s.detach().cpu().clone() for k, s in zip(names, self.shadow)},
                "updates": st["updates"], "decay": st["decay"], "weight": st["weight"]}

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        vals = list(sd["shadow"].values())
        if len(vals) != len(self.shadow):
            raise ValueError(f"WeightEma.load_state_dict: {len(vals)} tensors for {len(self.shadow)}")
        with torch.no_grad():
            for s, v in zip(self.shadow, vals):
                if tuple(v.shape) != tuple(s.shape):
                    raise ValueError(f"WeightEma.load_state_dict: shape {tuple(v.shape)} for {tuple(s.shape)}")
                s.copy_(v)
        self.state.write(sd)  # as stored: not rounded again
