"""Batch assembly from byte images (csrc/image_batch.hip): gather by index, normalise, random
crop + horizontal flip, ragged-tail padding and the targets, in ONE launch that writes the fp32
batch and its targets straight into their final tensors.

The reference loads CIFAR-10 through ``ToTensor + Normalize(0.5, 0.5)`` and a shuffling loader
(ddp_powersgd_guide_cifar10/ddp_init.py:40-58).  Here the images stay bytes in HBM and every
batch is produced by the rule below, identical bit for bit on device and in the torch twin.

The rule.  A sample has dataset index ``i``, epoch ``e``, loader seed ``s``, crop padding ``p``:

* ``scale_c = fp32(1 / (255 * std_c))``, ``shift_c = fp32(-mean_c / std_c)`` (host, fp64, rounded
  once); ``norm_c(v) = fmaf(float(v), scale_c, shift_c)``.  The torch twin evaluates
  ``double(v) * double(scale_c) + double(shift_c)`` (exact: 8 bits x 24 bits + 24 bits) and
  rounds once, which is the ``fmaf``;
* ``h = hash4(s, e, i, 0)``, ``h2 = hash4(s, e, i, 1)`` (all uint32; the attention dropout's
  counter hash); ``dx = (((h & 0xFFFF) * (2p+1)) >> 16) - p``, ``dy = (((h >> 16) * (2p+1)) >> 16)
  - p``, ``flip = h2 >> 31``; without augmentation ``dx = dy = flip = 0``;
* ``out[b, c, y, x] = norm_c(src[i, c, y + dy, (flip ? 31 - x : x) + dx])``, byte 0 outside the
  image: ``RandomCrop(32, padding=p)`` then the flip, before ``ToTensor``;
* ``target[b] = labels[i]``;
* rows ``b >= m`` (``m = len(idx)``) are zero images with ``target = pad_target``; so is a row
  whose index is outside ``[0, N)``, which is never dereferenced and sets ``err[0] = 1``.

The draw depends on ``(s, e, i)`` only: not on the batch size, the world size or the position.

Device tensors require the native kernel (no silent fallback); CPU tensors run the torch twin.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from ._ext import ext

__all__ = ["image_batch", "hash4", "crop_flip_draw", "image_norm_constants"]

_M = 0xFFFFFFFF


def hash4(a: int, b: int, c: int, d: int) -> int:
    """Python twin of the kernels' counter hash (csrc/counter_hash.h), uint32 arithmetic."""
    a, b, c, d = (int(v) & _M for v in (a, b, c, d))
    h = ((a * 0x9E3779B1) & _M) ^ ((((b + 0x7F4A7C15) & _M) * 0x85EBCA77) & _M)
    h ^= (((c + 0x165667B1) & _M) * 0xC2B2AE3D) & _M
    h = ((h ^ (h >> 15)) * 0x2C1B3C6D) & _M
    h ^= (((d + 0x27D4EB2F) & _M) * 0x9E3779B1) & _M
    h = ((h ^ (h >> 13)) * 0x297A2D39) & _M
    return h ^ (h >> 16)


def crop_flip_draw(seed: int, epoch: int, index: int, pad: int, flip: bool = True) -> Tuple[int, int, int]:
    """``(dx, dy, flip)`` of sample ``index`` in ``epoch`` under loader seed ``seed``."""
    h = hash4(seed, epoch, index, 0)
    span = 2 * int(pad) + 1
    dx = (((h & 0xFFFF) * span) >> 16) - int(pad)
    dy = (((h >> 16) * span) >> 16) - int(pad)
    return dx, dy, (hash4(seed, epoch, index, 1) >> 31) if flip else 0


def image_norm_constants(mean: Sequence[float], std: Sequence[float]) -> Tuple[list, list]:
    """``(scale, shift)`` per channel: fp64 on the host, rounded once to fp32 (returned as the
    Python floats that hold those fp32 values exactly)."""
    if len(mean) != len(std):
        raise ValueError("image_batch: mean and std need one entry per channel each")
    scale = [float(np.float32(1.0 / (255.0 * float(s)))) for s in std]
    shift = [float(np.float32(-float(m) / float(s))) for m, s in zip(mean, std)]
    return scale, shift


def _mul32(a: torch.Tensor, c: int) -> torch.Tensor:
    """(a * c) mod 2^32 for int64 tensors holding uint32 values, without int64 overflow."""
    return ((a & 0xFFFF) * c + ((((a >> 16) * c) & 0xFFFF) << 16)) & _M


def _hash4_t(a: int, b: int, c: torch.Tensor, d: int) -> torch.Tensor:
    """:func:`hash4` over an int64 tensor ``c`` of uint32 values."""
    h0 = ((int(a) & _M) * 0x9E3779B1 & _M) ^ ((((int(b) & _M) + 0x7F4A7C15) & _M) * 0x85EBCA77 & _M)
    h = h0 ^ _mul32((c + 0x165667B1) & _M, 0xC2B2AE3D)
    h = _mul32(h ^ (h >> 15), 0x2C1B3C6D)
    h = h ^ ((((int(d) & _M) + 0x27D4EB2F) & _M) * 0x9E3779B1 & _M)
    h = _mul32(h ^ (h >> 13), 0x297A2D39)
    return h ^ (h >> 16)


def _torch_image_batch(src, labels, idx, out, out_target, m, B, scale, shift, pad, flip, seed, epoch, pad_target,
                       err) -> None:
    """The rule of the module docstring in tensor ops (CPU)."""
    N, C = int(src.shape[0]), int(src.shape[1])
    i = idx[:m].long()
    valid = (i >= 0) & (i < N)
    safe = torch.where(valid, i, torch.zeros_like(i))
    u = safe & _M
    if pad > 0:
        h = _hash4_t(seed, epoch, u, 0)
        span = 2 * pad + 1
        dx = (((h & 0xFFFF) * span) >> 16) - pad
        dy = (((h >> 16) * span) >> 16) - pad
    else:
        dx = dy = torch.zeros_like(u)
    fl = (_hash4_t(seed, epoch, u, 1) >> 31).bool() if flip else torch.zeros_like(u, dtype=torch.bool)
    ar = torch.arange(32, dtype=torch.int64)
    sy = ar[None, :] + dy[:, None]                                             # [m, 32]
    sx = torch.where(fl[:, None], 31 - ar[None, :], ar[None, :]) + dx[:, None]  # [m, 32]
    inb = (((sy >= 0) & (sy < 32))[:, :, None] & ((sx >= 0) & (sx < 32))[:, None, :])[:, None]  # [m, 1, 32, 32]
    planes = src.index_select(0, safe)                                          # [m, C, 32, 32]
    rows = planes.gather(2, sy.clamp(0, 31)[:, None, :, None].expand(m, C, 32, 32))
    px = rows.gather(3, sx.clamp(0, 31)[:, None, None, :].expand(m, C, 32, 32))
    v = torch.where(inb, px, torch.zeros_like(px)).double()
    sc = torch.tensor(scale, dtype=torch.float64).view(1, C, 1, 1)
    sh = torch.tensor(shift, dtype=torch.float64).view(1, C, 1, 1)
    img = (v * sc + sh).float()
    out[:m] = torch.where(valid[:, None, None, None], img, torch.zeros_like(img))
    out_target[:m] = torch.where(valid, labels.index_select(0, safe), torch.full_like(safe, pad_target))
    if m < B:
        out[m:B] = 0
        out_target[m:B] = pad_target
    if not bool(valid.all()):
        err.fill_(1)


def image_batch(src: torch.Tensor, labels: torch.Tensor, idx: torch.Tensor, *, out: Optional[torch.Tensor] = None,
                out_target: Optional[torch.Tensor] = None, rows: Optional[int] = None, mean: Sequence[float],
                std: Sequence[float], pad: int = 0, flip: bool = False, seed: int = 0, epoch: int = 0,
                pad_target: int = -100, err: Optional[torch.Tensor] = None):
    """``(out, out_target)``: the first ``rows`` rows of ``out`` (fp32 ``[>= rows, C, 32, 32]``)
    and ``out_target`` (int64) are written by the module's rule from ``src`` (uint8 ``[N, C, 32,
    32]``), ``labels`` (int64 ``[N]``) and ``idx`` (int64 ``[m]``, ``1 <= m <= rows``).  ``rows``
    defaults to the rows of ``out``, or to ``m`` when ``out`` is created here.  ``err`` (int32,
    optional) is set to 1 when an index is outside ``[0, N)``; it is never cleared here."""
    if src.dtype != torch.uint8 or src.dim() != 4 or tuple(src.shape[2:]) != (32, 32):
        raise ValueError(f"image_batch: src must be uint8 [N, C, 32, 32], got {src.dtype} {tuple(src.shape)}")
    N, C = int(src.shape[0]), int(src.shape[1])
    if labels.dtype != torch.int64 or labels.dim() != 1 or labels.shape[0] != N:
        raise ValueError("image_batch: labels must be int64 [N]")
    if idx.dtype != torch.int64 or idx.dim() != 1:
        raise ValueError("image_batch: idx must be int64 [m]")
    m = int(idx.shape[0])
    if len(mean) != C or len(std) != C:
        raise ValueError(f"image_batch: mean / std need {C} entries")
    if not 0 <= int(pad) <= 8:
        raise ValueError("image_batch: 0 <= pad <= 8 required")
    B = int(rows) if rows is not None else (int(out.shape[0]) if out is not None else m)
    if not 1 <= m <= B:
        raise ValueError(f"image_batch: 1 <= len(idx) <= rows required (len(idx) = {m}, rows = {B})")
    dev = src.device
    if out is None:
        out = torch.empty((B, C, 32, 32), dtype=torch.float32, device=dev)
    if out_target is None:
        out_target = torch.empty((B,), dtype=torch.int64, device=dev)
    if (out.dtype != torch.float32 or tuple(out.shape[1:]) != (C, 32, 32) or out.shape[0] < B
            or not out.is_contiguous()):
        raise ValueError(f"image_batch: out must be contiguous float32 [>= {B}, {C}, 32, 32]")
    if (out_target.dtype != torch.int64 or out_target.dim() != 1 or out_target.shape[0] < B
            or not out_target.is_contiguous()):
        raise ValueError(f"image_batch: out_target must be contiguous int64 [>= {B}]")
    if err is None:
        err = torch.zeros(1, dtype=torch.int32, device=dev)
    if err.dtype != torch.int32 or err.numel() < 1:
        raise ValueError("image_batch: err must be an int32 tensor")
    for name, t in (("labels", labels), ("idx", idx), ("out", out), ("out_target", out_target), ("err", err)):
        if t.device != dev:
            raise ValueError(f"image_batch: {name} is on {t.device}, src on {dev}")
    scale, shift = image_norm_constants(mean, std)
    if src.is_cuda:
        ext().image_batch(src.contiguous(), labels.contiguous(), idx.contiguous(), out, out_target, m, B, scale,
                          shift, int(pad), bool(flip), int(seed) & _M, int(epoch) & _M, int(pad_target), err)
    else:
        _torch_image_batch(src, labels, idx, out, out_target, m, B, scale, shift, int(pad), bool(flip),
                           int(seed), int(epoch), int(pad_target), err)
    return out, out_target
