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

:func:`image_mix_batch` is the same batch with mixup / CutMix against the reversed batch, a kernel
of its own with its own twin; its docstring holds the mixing rule.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from ._ext import ext

__all__ = ["image_batch", "image_mix_batch", "hash4", "crop_flip_draw", "mix_draw", "image_norm_constants",
           "MIX_MODES"]

_M = 0xFFFFFFFF
MIX_MODES = {"mixup": 1, "cutmix": 2, "mixup_cutmix": 3}  # the kernel's mode argument


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


def _mix_mode(mode: str, mix_prob: float) -> Tuple[int, int]:
    """``(kernel mode, thr)``; ``thr = int(mix_prob * 2^24)``: a row is drawn when its 24-bit hash is below it."""
    if mode not in MIX_MODES:
        raise ValueError(f"mix mode {mode!r}; allowed: {sorted(MIX_MODES)}")
    if not 0.0 < float(mix_prob) <= 1.0:  # NaN fails the comparison too
        raise ValueError(f"mix_prob = {mix_prob} must lie in (0, 1]")
    thr = int(float(mix_prob) * (1 << 24))
    if thr < 1:
        raise ValueError(f"mix_prob = {mix_prob} is below 2^-24, the resolution of the draw")
    return MIX_MODES[mode], thr


def mix_draw(seed: int, epoch: int, index: int, mode: str, mix_prob: float = 1.0):
    """``(mixed_by_hash, kind, lam, box)`` of sample ``index`` in ``epoch`` under loader seed
    ``seed``: whether the hash draws the row for mixing (its place in the batch decides the
    partner, and the centre row of an odd batch stays unmixed whatever the hash says), ``kind`` =
    ``"mixup"`` / ``"cutmix"``, the weight ``lam`` of the row's own label, and the CutMix box
    ``(x0, y0, x1, y1)`` in output coordinates (``None`` for mixup).  An undrawn row gives
    ``(False, None, 1.0, None)``."""
    code, thr = _mix_mode(mode, mix_prob)
    h3 = hash4(seed, epoch, index, 2)
    if not (h3 >> 8) < thr:
        return False, None, 1.0, None
    h4 = hash4(seed, epoch, index, 3)
    if code == 2 or (code == 3 and (h3 & 1)):
        h5 = hash4(seed, epoch, index, 4)
        side = math.isqrt(h4 >> 16) >> 3
        cx, cy = ((h5 & 0xFFFF) * 32) >> 16, ((h5 >> 16) * 32) >> 16
        x0, x1 = max(cx - (side >> 1), 0), min(cx - (side >> 1) + side, 32)
        y0, y1 = max(cy - (side >> 1), 0), min(cy - (side >> 1) + side, 32)
        return True, "cutmix", (1024 - (x1 - x0) * (y1 - y0)) / 1024.0, (x0, y0, x1, y1)
    return True, "mixup", (h4 >> 8) / float(1 << 24), None


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


def _torch_rows(src, safe, scale, shift, pad, flip, seed, epoch) -> torch.Tensor:
    """``[m, C, 32, 32]`` fp32: the samples ``safe`` (indices inside ``[0, N)``) normalised, each
    with its own crop / flip draw."""
    m, C = int(safe.shape[0]), int(src.shape[1])
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
    return (v * sc + sh).float()


def _torch_image_batch(src, labels, idx, out, out_target, m, B, scale, shift, pad, flip, seed, epoch, pad_target,
                       err) -> None:
    """The rule of the module docstring in tensor ops (CPU)."""
    N = int(src.shape[0])
    i = idx[:m].long()
    valid = (i >= 0) & (i < N)
    safe = torch.where(valid, i, torch.zeros_like(i))
    img = _torch_rows(src, safe, scale, shift, pad, flip, seed, epoch)
    out[:m] = torch.where(valid[:, None, None, None], img, torch.zeros_like(img))
    out_target[:m] = torch.where(valid, labels.index_select(0, safe), torch.full_like(safe, pad_target))
    if m < B:
        out[m:B] = 0
        out_target[m:B] = pad_target
    if not bool(valid.all()):
        err.fill_(1)


def _prepare(fn, src, labels, idx, out, out_target, rows, mean, std, pad, err):
    """The argument checks of :func:`image_batch`; creates ``out`` / ``out_target`` / ``err`` where absent.
    Returns ``(m, B, out, out_target, err)``."""
    if src.dtype != torch.uint8 or src.dim() != 4 or tuple(src.shape[2:]) != (32, 32):
        raise ValueError(f"{fn}: src must be uint8 [N, C, 32, 32], got {src.dtype} {tuple(src.shape)}")
    N, C = int(src.shape[0]), int(src.shape[1])
    if labels.dtype != torch.int64 or labels.dim() != 1 or labels.shape[0] != N:
        raise ValueError(f"{fn}: labels must be int64 [N]")
    if idx.dtype != torch.int64 or idx.dim() != 1:
        raise ValueError(f"{fn}: idx must be int64 [m]")
    m = int(idx.shape[0])
    if len(mean) != C or len(std) != C:
        raise ValueError(f"{fn}: mean / std need {C} entries")
    if not 0 <= int(pad) <= 8:
        raise ValueError(f"{fn}: 0 <= pad <= 8 required")
    B = int(rows) if rows is not None else (int(out.shape[0]) if out is not None else m)
    if not 1 <= m <= B:
        raise ValueError(f"{fn}: 1 <= len(idx) <= rows required (len(idx) = {m}, rows = {B})")
    dev = src.device
    if out is None:
        out = torch.empty((B, C, 32, 32), dtype=torch.float32, device=dev)
    if out_target is None:
        out_target = torch.empty((B,), dtype=torch.int64, device=dev)
    if (out.dtype != torch.float32 or tuple(out.shape[1:]) != (C, 32, 32) or out.shape[0] < B
            or not out.is_contiguous()):
        raise ValueError(f"{fn}: out must be contiguous float32 [>= {B}, {C}, 32, 32]")
    if (out_target.dtype != torch.int64 or out_target.dim() != 1 or out_target.shape[0] < B
            or not out_target.is_contiguous()):
        raise ValueError(f"{fn}: out_target must be contiguous int64 [>= {B}]")
    if err is None:
        err = torch.zeros(1, dtype=torch.int32, device=dev)
    if err.dtype != torch.int32 or err.numel() < 1:
        raise ValueError(f"{fn}: err must be an int32 tensor")
    for name, t in (("labels", labels), ("idx", idx), ("out", out), ("out_target", out_target), ("err", err)):
        if t.device != dev:
            raise ValueError(f"{fn}: {name} is on {t.device}, src on {dev}")
    return m, B, out, out_target, err


def image_batch(src: torch.Tensor, labels: torch.Tensor, idx: torch.Tensor, *, out: Optional[torch.Tensor] = None,
                out_target: Optional[torch.Tensor] = None, rows: Optional[int] = None, mean: Sequence[float],
                std: Sequence[float], pad: int = 0, flip: bool = False, seed: int = 0, epoch: int = 0,
                pad_target: int = -100, err: Optional[torch.Tensor] = None):
    """``(out, out_target)``: the first ``rows`` rows of ``out`` (fp32 ``[>= rows, C, 32, 32]``)
    and ``out_target`` (int64) are written by the module's rule from ``src`` (uint8 ``[N, C, 32,
    32]``), ``labels`` (int64 ``[N]``) and ``idx`` (int64 ``[m]``, ``1 <= m <= rows``).  ``rows``
    defaults to the rows of ``out``, or to ``m`` when ``out`` is created here.  ``err`` (int32,
    optional) is set to 1 when an index is outside ``[0, N)``; it is never cleared here."""
    m, B, out, out_target, err = _prepare("image_batch", src, labels, idx, out, out_target, rows, mean, std, pad,
                                          err)
    scale, shift = image_norm_constants(mean, std)
    if src.is_cuda:
        ext().image_batch(src.contiguous(), labels.contiguous(), idx.contiguous(), out, out_target, m, B, scale,
                          shift, int(pad), bool(flip), int(seed) & _M, int(epoch) & _M, int(pad_target), err)
    else:
        _torch_image_batch(src, labels, idx, out, out_target, m, B, scale, shift, int(pad), bool(flip),
                           int(seed), int(epoch), int(pad_target), err)
    return out, out_target


def _torch_image_mix_batch(src, labels, idx, out, out_target, out_target_b, out_lam, m, B, scale, shift, pad, flip,
                           seed, epoch, pad_target, err, mode, thr) -> None:
    """The mixing rule of :func:`image_mix_batch` in tensor ops (CPU)."""
    N = int(src.shape[0])
    i = idx[:m].long()
    j = i.flip(0)  # row b's partner is row m - 1 - b
    valid = (i >= 0) & (i < N)
    partner_ok = (j >= 0) & (j < N)
    safe = torch.where(valid, i, torch.zeros_like(i))
    safe_j = torch.where(partner_ok, j, torch.zeros_like(j))
    u = safe & _M
    h3 = _hash4_t(seed, epoch, u, 2)
    pos = torch.arange(m, dtype=torch.int64)
    mixed = ((h3 >> 8) < thr) & (pos != m - 1 - pos) & partner_ok & valid
    cut = mixed & (torch.ones_like(mixed) if mode == 2 else ((h3 & 1) == 1) if mode == 3 else torch.zeros_like(mixed))
    h4 = _hash4_t(seed, epoch, u, 3)
    h5 = _hash4_t(seed, epoch, u, 4)
    va = _torch_rows(src, safe, scale, shift, pad, flip, seed, epoch)
    vb = _torch_rows(src, safe_j, scale, shift, pad, flip, seed, epoch)
    # mixup: three fp32 operations, each rounded (tensor ops never contract into an fma)
    lam_mix = (h4 >> 8).float() * (1.0 / (1 << 24))
    lm = lam_mix[:, None, None, None]
    blended = lm * va + (1.0 - lm) * vb
    # CutMix: an integer box, a select
    w = h4 >> 16
    r = torch.sqrt(w.double()).floor().long()
    r = r - (r * r > w).long()
    r = r + ((r + 1) * (r + 1) <= w).long()
    side = r >> 3
    cx, cy = ((h5 & 0xFFFF) * 32) >> 16, ((h5 >> 16) * 32) >> 16
    x0, x1 = (cx - (side >> 1)).clamp(min=0), (cx - (side >> 1) + side).clamp(max=32)
    y0, y1 = (cy - (side >> 1)).clamp(min=0), (cy - (side >> 1) + side).clamp(max=32)
    ar = torch.arange(32, dtype=torch.int64)
    in_x = (ar[None, :] >= x0[:, None]) & (ar[None, :] < x1[:, None])  # [m, 32]
    in_y = (ar[None, :] >= y0[:, None]) & (ar[None, :] < y1[:, None])
    box = (in_y[:, :, None] & in_x[:, None, :])[:, None]                # [m, 1, 32, 32]
    lam_cut = (1024 - (x1 - x0) * (y1 - y0)).float() * (1.0 / 1024.0)
    img = torch.where(cut[:, None, None, None], torch.where(box, vb, va),
                      torch.where(mixed[:, None, None, None], blended, va))
    lam = torch.where(cut, lam_cut, torch.where(mixed, lam_mix, torch.ones_like(lam_mix)))
    own = labels.index_select(0, safe)
    pad_t = torch.full_like(safe, pad_target)
    out[:m] = torch.where(valid[:, None, None, None], img, torch.zeros_like(img))
    out_target[:m] = torch.where(valid, own, pad_t)
    out_target_b[:m] = torch.where(valid, torch.where(mixed, labels.index_select(0, safe_j), own), pad_t)
    out_lam[:m] = lam
    if m < B:
        out[m:B] = 0
        out_target[m:B] = pad_target
        out_target_b[m:B] = pad_target
        out_lam[m:B] = 1.0
    if not bool(valid.all()):  # a bad partner index is some row's bad own index
        err.fill_(1)


def image_mix_batch(src: torch.Tensor, labels: torch.Tensor, idx: torch.Tensor, *, mode: str, mix_prob: float = 1.0,
                    out: Optional[torch.Tensor] = None, out_target: Optional[torch.Tensor] = None,
                    out_target_b: Optional[torch.Tensor] = None, out_lam: Optional[torch.Tensor] = None,
                    rows: Optional[int] = None, mean: Sequence[float], std: Sequence[float], pad: int = 0,
                    flip: bool = False, seed: int = 0, epoch: int = 0, pad_target: int = -100,
                    err: Optional[torch.Tensor] = None):
    """``(out, out_target, out_target_b, out_lam)``: :func:`image_batch` with mixup / CutMix
    (csrc/image_batch.hip: ``image_mix_batch_kernel``, one launch; bitwise the torch twin).

    Row ``b < m`` with sample ``i = idx[b]`` has the partner ``b' = m - 1 - b``, ``j = idx[b']``
    (the batch reversed).  ``h3 = hash4(s, e, i, 2)``; the row is mixed iff ``(h3 >> 8) <
    int(mix_prob * 2^24)``, ``b' != b`` and ``0 <= j < N`` (a bad partner index is never
    dereferenced and sets ``err``).  ``mode``: ``"mixup"``, ``"cutmix"`` or ``"mixup_cutmix"``
    (CutMix iff ``h3 & 1``).  ``va`` / ``vb`` are :func:`image_batch`'s pixels of ``i`` / ``j``,
    each with its own crop and flip draw; with ``h4 = hash4(s, e, i, 3)``, ``h5 = hash4(s, e, i, 4)``:

    * mixup: ``lam = float(h4 >> 8) * 2^-24``, ``out = fl(fl(lam * va) + fl((1 - lam) * vb))``;
    * CutMix: ``side = isqrt(h4 >> 16) >> 3``, centre ``cx = ((h5 & 0xFFFF) * 32) >> 16``, ``cy =
      ((h5 >> 16) * 32) >> 16``, box ``[max(c - side // 2, 0), min(c - side // 2 + side, 32))``
      per axis in output coordinates; ``out = vb`` inside, ``va`` outside; ``lam = (1024 - box
      area) / 1024``;
    * unmixed: ``out = va`` (bitwise :func:`image_batch`), ``lam = 1``, ``target_b = target``.

    ``out_target[b] = labels[i]``, ``out_target_b[b] = labels[j]`` when mixed, ``out_lam[b] =
    lam`` (fp32): the loss is ``lam * ce(target) + (1 - lam) * ce(target_b)``.  Padding rows and
    rows with a bad own index are zero images with both targets ``pad_target`` and ``lam = 1``.
    :func:`mix_draw` gives one sample's draw.  It depends on ``(s, e, i)`` only; the partner
    depends on the batch's composition."""
    code, thr = _mix_mode(mode, mix_prob)
    m, B, out, out_target, err = _prepare("image_mix_batch", src, labels, idx, out, out_target, rows, mean, std, pad,
                                          err)
    dev = src.device
    if out_target_b is None:
        out_target_b = torch.empty((B,), dtype=torch.int64, device=dev)
    if out_lam is None:
        out_lam = torch.empty((B,), dtype=torch.float32, device=dev)
    for name, t, dtype in (("out_target_b", out_target_b, torch.int64), ("out_lam", out_lam, torch.float32)):
        if t.dtype != dtype or t.dim() != 1 or t.shape[0] < B or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"image_mix_batch: {name} must be contiguous {dtype} [>= {B}] on {dev}")
    scale, shift = image_norm_constants(mean, std)
    if src.is_cuda:
        ext().image_mix_batch(src.contiguous(), labels.contiguous(), idx.contiguous(), out, out_target, out_target_b,
                              out_lam, m, B, scale, shift, int(pad), bool(flip), int(seed) & _M, int(epoch) & _M,
                              int(pad_target), err, code, thr)
    else:
        _torch_image_mix_batch(src, labels, idx, out, out_target, out_target_b, out_lam, m, B, scale, shift, int(pad),
                               bool(flip), int(seed), int(epoch), int(pad_target), err, code, thr)
    return out, out_target, out_target_b, out_lam
