"""Fused softmax cross-entropy on gfx950 (csrc/loss.hip), a drop-in for
``torch.nn.CrossEntropyLoss()`` / ``F.cross_entropy`` with the reference's settings (mean
reduction, ``ignore_index=-100``, no class weights), plus label smoothing and a second, weighted
target per row (mixup / CutMix: ``lam * ce(target) + (1 - lam) * ce(target_b)``).

The reference computes its training loss with ``nn.CrossEntropyLoss`` (e.g.
ddp_powersgd_guide_cifar10/ddp_init.py:145; HF DistilBERT's classification head for the
IMDb workload).  PyTorch-ROCm lowers that to log_softmax + nll_loss forward and a zero fill
+ nll_loss_backward + log_softmax_backward: 5 launches per step, ~30 µs of a ResNet-18
step at per-GPU batch 64 (profiles/r2/).  Here it is one forward launch — row losses, the
saved gradient ``softmax - onehot`` and a fixed-order mean by the last workgroup — and one
backward launch that scales the saved gradient.  ``label_smoothing != 0`` or a second target
take ``ce_soft_fwd_kernel``, the same launch shape with one more wave sum per row and the same
scratch layout, so the backward launch is shared; the default call stays on ``ce_fwd_kernel`` and is
bitwise what it was.  CPU tensors and other settings (class weights, other reductions) fall back
to ``F.cross_entropy``; on device the native path is required (no silent fallback).
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._ext import ext
from ..knobs import fusion_on

__all__ = ["cross_entropy", "CrossEntropyLoss"]

_CTR: dict = {}
_ENABLED = fusion_on("fused_ce")  # =0: PyTorch-ROCm's loss kernels (A/B)


def _counter(device: torch.device) -> torch.Tensor:
    """The kernel's last-workgroup counter, re-armed to 0 by every launch.  One per device:
    per-stream counters would be created inside a graph capture (the warm-up runs on another
    stream) and cost a memset node per replay; the framework never runs two losses of one
    device concurrently."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    c = _CTR.get(idx)
    if c is None:  # first use is eager (warm-up), never inside a capture
        c = _CTR[idx] = torch.zeros(1, dtype=torch.int32, device=device)
    return c


class _CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, ignore_index, acc=None):
        x = logits.contiguous()
        t = target.contiguous()
        dl = torch.empty_like(x)
        scratch = torch.empty(x.shape[0] + 1, device=x.device, dtype=torch.float32)
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        ext().ce_fwd(x, t, dl, scratch, loss, _counter(x.device), int(ignore_index), acc)
        ctx.save_for_backward(dl, scratch)
        return loss

    @staticmethod
    def backward(ctx, g):
        dl, scratch = ctx.saved_tensors
        dx = torch.empty_like(dl)
        ext().ce_bwd(dl, g.reshape(1).contiguous().float(), scratch, dx)
        return dx, None, None, None


class _SoftCrossEntropyFn(torch.autograd.Function):
    """``ce_soft_fwd_kernel``: label smoothing ``eps`` and an optional ``(target_b, lam)``; the saved
    gradient and scratch have ``_CrossEntropyFn``'s layout, so the backward launch is the same."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index, acc, eps, target_b, lam):
        x = logits.contiguous()
        dl = torch.empty_like(x)
        scratch = torch.empty(x.shape[0] + 1, device=x.device, dtype=torch.float32)
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        ext().ce_soft_fwd(x, target.contiguous(), dl, scratch, loss, _counter(x.device), int(ignore_index),
                          float(eps), None if target_b is None else target_b.contiguous(),
                          None if lam is None else lam.contiguous(), acc)
        ctx.save_for_backward(dl, scratch)
        return loss

    @staticmethod
    def backward(ctx, g):
        dl, scratch = ctx.saved_tensors
        dx = torch.empty_like(dl)
        ext().ce_bwd(dl, g.reshape(1).contiguous().float(), scratch, dx)
        return dx, None, None, None, None, None, None


def _torch_soft_cross_entropy(logits, target, ignore_index, eps, target_b, lam):
    """The soft loss as a torch composition: mean over the rows whose ``target`` is not ignored."""
    if target_b is None:
        return F.cross_entropy(logits, target, ignore_index=ignore_index, label_smoothing=eps)
    la = F.cross_entropy(logits, target, ignore_index=ignore_index, label_smoothing=eps, reduction="none")
    lb = F.cross_entropy(logits, target_b, ignore_index=ignore_index, label_smoothing=eps, reduction="none")
    lam = lam.to(la.dtype)
    valid = target != ignore_index
    rows = torch.where(valid, lam * la + (1.0 - lam) * lb, torch.zeros_like(la))
    return rows.sum() / valid.sum().to(la.dtype)


def cross_entropy(logits: torch.Tensor, target: torch.Tensor, ignore_index: int = -100,
                  accumulate: "torch.Tensor | None" = None, label_smoothing: float = 0.0,
                  target_b: "torch.Tensor | None" = None, lam: "torch.Tensor | None" = None) -> torch.Tensor:
    """``accumulate`` (optional one-element fp32 tensor): ``accumulate += loss`` as well (a
    running loss sum for logging; inside the kernel on device, no separate add launch).

    ``label_smoothing`` is ``torch.nn.CrossEntropyLoss``'s.  ``target_b`` (int64 ``[B]``) with
    ``lam`` (fp32 ``[B]``) mixes two targets per row, ``lam * ce(target) + (1 - lam) *
    ce(target_b)``, each smoothed; a row counts iff ``target != ignore_index``.  With
    ``label_smoothing == 0`` and no ``target_b`` the call is the plain one, bitwise."""
    if (target_b is None) != (lam is None):
        raise ValueError("cross_entropy: target_b and lam come together")
    eps = float(label_smoothing)
    if not 0.0 <= eps < 1.0:  # NaN fails the comparison too
        raise ValueError(f"cross_entropy: label_smoothing = {label_smoothing} must lie in [0, 1)")
    native = (_ENABLED and logits.is_cuda and logits.dim() == 2 and logits.dtype == torch.float32
              and target.dtype == torch.int64 and target.dim() == 1 and logits.shape[0] >= 1)
    if eps != 0.0 or target_b is not None:
        if native:
            if target_b is not None and (target_b.dtype != torch.int64 or target_b.shape != target.shape
                                         or lam.dtype != torch.float32 or lam.shape != target.shape):
                raise ValueError("cross_entropy: target_b must be int64 and lam float32, both shaped like target")
            return _SoftCrossEntropyFn.apply(logits, target, ignore_index, accumulate, eps, target_b, lam)
        loss = _torch_soft_cross_entropy(logits, target, ignore_index, eps, target_b, lam)
        if accumulate is not None:
            accumulate.add_(loss.detach())
        return loss
    if native:
        return _CrossEntropyFn.apply(logits, target, ignore_index, accumulate)
    loss = F.cross_entropy(logits, target, ignore_index=ignore_index)
    if accumulate is not None:
        accumulate.add_(loss.detach())
    return loss


class CrossEntropyLoss(nn.CrossEntropyLoss):
    """``nn.CrossEntropyLoss`` whose mean reduction without class weights runs the fused kernels on
    device, ``label_smoothing`` included; ``forward`` also takes a mixed batch's ``target_b`` / ``lam``."""

    # optional running loss sum (``cross_entropy(accumulate=)``), e.g. the trainer's epoch loss
    accumulate: "torch.Tensor | None" = None

    def forward(self, input: torch.Tensor, target: torch.Tensor, target_b: "torch.Tensor | None" = None,
                lam: "torch.Tensor | None" = None) -> torch.Tensor:
        if self.weight is None and self.reduction == "mean":
            return cross_entropy(input, target, self.ignore_index, self.accumulate, self.label_smoothing, target_b,
                                 lam)
        if target_b is not None:
            raise ValueError("CrossEntropyLoss: target_b / lam need weight=None and reduction='mean'")
        loss = super().forward(input, target)
        if self.accumulate is not None:
            self.accumulate.add_(loss.detach())
        return loss
