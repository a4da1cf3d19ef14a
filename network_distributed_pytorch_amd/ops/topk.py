"""Top-k gradient sparsification with error feedback on gfx950 (csrc/topk.hip): the exact global
top-k of ``m = g + e`` over a flat arena in five launches (a three-pass radix select of the k-th
largest magnitude, a count and an ordered compact), and the owner-computes decompress + momentum +
SGD update behind the all-gather in one more.

The rule (exact: bitwise identical on the device and in the torch twin that CPU tensors run), over
flat fp32 arenas of ``n`` elements ``g`` (gradient), ``e`` (error memory), ``x`` (weights), ``b``
(momentum) and ``1 <= k <= n``:

1. ``m_i = fadd(g_i, e_i)``; ``key_i = bits(m_i) & 0x7fffffff``, the magnitude as a 31-bit unsigned
   integer: NaN sorts above inf (a NaN is selected and reaches every replica), ``-0`` has key 0.
2. ``T`` = the k-th largest key counted with multiplicity, ``c = #{key > T}``.  Selected: every
   ``i`` with ``key_i > T`` plus the first ``k - c`` indices, ascending, with ``key_i == T``:
   exactly ``k`` entries.  Output ``int32[2k]``: ``idx`` ascending, then ``bits(m_idx)``.
3. ``e_i' = 0`` where selected, ``m_i`` elsewhere.
4. The ranks' outputs are gathered into ``[N, 2k]`` (one all-gather; none with ``N = 1``).
5. Per element ``acc = 0``; for ``r = 0 .. N-1`` in rank order, if rank ``r`` selected ``i``:
   ``acc = fadd(acc, val_r)``; ``o = acc / N`` when ``N != 1`` else ``acc``; then the PowerSGD
   element rule: ``d = (wd != 0) ? fmaf(wd, x, o) : o``; ``b' = fadd(fmul(b, lambda), d)``;
   ``up = fadd(d, b')``; ``x' = fmaf(-lr, up, x)``.

Device tensors run the native kernels, CPU tensors the twin; a device tensor the kernels cannot
take (not fp32, not contiguous) is an error, never a fallback.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ._ext import ext

__all__ = ["TopKCore", "topk_count", "fmaf32"]

_KEY = 0x7FFFFFFF


def topk_count(numel: int, ratio: float, n: Optional[int] = None) -> int:
    """``k = max(1, ceil(ratio * numel))``, capped at the arena size ``n``."""
    if not 0.0 < float(ratio) <= 1.0:
        raise ValueError(f"top-k: topk_ratio must be in (0, 1], got {ratio}")
    k = max(1, int(np.ceil(float(ratio) * int(numel))))
    return min(k, int(numel if n is None else n))


def fmaf32(a, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """``fmaf(a, b, c)`` on fp32 values, correctly rounded once: the product is exact in fp64, the
    sum is rounded to odd there (its TwoSum residual decides the sticky bit) and then to fp32."""
    p = torch.as_tensor(a, dtype=torch.float32).double() * b.double()
    c = c.double()
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    bits = s.contiguous().view(torch.int64)
    fix = (err != 0) & torch.isfinite(s) & ((bits & 1) == 0)
    away = (err > 0) == (s > 0)  # the exact sum lies further from zero than s
    bits = torch.where(fix, bits + torch.where(away, 1, -1), bits)
    return bits.view(torch.float64).float()


class TopKCore:
    """Scratch, device block, output and gathered buffers of one top-k compressor over arenas of
    ``n`` elements; everything is allocated here, before any capture.  ``out`` is this rank's
    ``int32[2k]`` (``idx | bits(val)``), ``gathered`` the ``[world, 2k]`` the update reads (``out``
    itself when ``world == 1``)."""

    def __init__(self, device, n: int, k: int, world: int = 1):
        self.device = torch.device(device)
        self.n, self.k, self.world = int(n), int(k), int(world)
        if not (1 <= self.k <= self.n < 2 ** 31):
            raise ValueError(f"top-k: 1 <= k <= n < 2^31 required, got k = {k}, n = {n}")
        if self.world < 1:
            raise ValueError(f"top-k: world >= 1 required, got {world}")
        i32 = dict(dtype=torch.int32, device=self.device)
        self.out = torch.zeros(2 * self.k, **i32)
        self.gathered = self.out.view(1, -1) if self.world == 1 else torch.zeros(self.world, 2 * self.k, **i32)
        self.block = None  # {prefix, krem, T, c, ties, 0, 0, 0}: rewritten by every select
        if self.device.type == "cuda":
            assert not torch.cuda.is_current_stream_capturing(), "TopKCore is built before capture"
            self.scratch = torch.zeros(ext().topk_scratch_words(self.n), **i32)
            self.block = torch.zeros(8, **i32)

    def _check(self, *tensors):
        for t in tensors:
            if t.device != self.device:
                raise ValueError(f"TopKCore on {self.device}: tensor on {t.device}")
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != self.n:
                raise ValueError(f"TopKCore: arenas must be contiguous float32 of {self.n} elements "
                                 f"(got {t.dtype}, contiguous={t.is_contiguous()}, numel={t.numel()})")

    def select(self, g: torch.Tensor, e: torch.Tensor, stage: int = -1) -> torch.Tensor:
        """Steps 1-3: ``e`` becomes the residual, ``out`` the selection; returns ``out``.  ``stage``
        0..4 runs one of the five device launches alone (profiling)."""
        self._check(g, e)
        if self.device.type == "cuda":
            ext().topk_select(g, e, self.k, self.scratch, self.block, self.out, stage)
            return self.out
        torch.add(g, e, out=e)
        key = e.view(torch.int32) & _KEY
        T = torch.kthvalue(key, self.n - self.k + 1).values
        above = torch.nonzero(key > T).reshape(-1)
        ties = torch.nonzero(key == T).reshape(-1)[: self.k - above.numel()]
        idx = torch.cat([above, ties]).sort().values
        self.out[: self.k] = idx.to(torch.int32)
        self.out[self.k:] = e.view(torch.int32)[idx]
        e[idx] = 0.0
        return self.out

    def update(self, x: torch.Tensor, b: torch.Tensor, gathered: torch.Tensor, lr: float, lam: float,
               wd: float = 0.0, hyper: Optional[torch.Tensor] = None) -> None:
        """Step 5 over ``gathered`` (``int32 [world, 2k]``).  On a device ``lr`` goes by value and
        there is no decay unless ``hyper``, the block ``[lr, weight_decay, 0, 0]``, is given (then
        ``lr`` / ``wd`` here are ignored)."""
        self._check(x, b)
        N, k = self.world, self.k
        if gathered.dtype != torch.int32 or gathered.numel() != N * 2 * k or not gathered.is_contiguous():
            raise ValueError(f"TopKCore.update: gathered must be contiguous int32 [{N}, {2 * k}]")
        if self.device.type == "cuda":
            if hyper is None and wd != 0.0:
                raise ValueError("TopKCore.update: weight decay on the device goes through the hyper block")
            ext().topk_update(x, b, gathered, k, N, float(lr), float(lam), hyper)
            return
        o = self._decode(gathered)
        lr, lam, wd = (float(np.float32(v)) for v in (lr, lam, wd))
        d = fmaf32(wd, x, o) if wd != 0 else o
        b.copy_(b * lam + d)
        x.copy_(fmaf32(-lr, d + b, x))

    def _decode(self, gathered: torch.Tensor) -> torch.Tensor:
        """The twin's ``o`` of step 5, ``[n]``: the rank-ordered sum of the selected values, over ``N``."""
        N, k = self.world, self.k
        rows = gathered.view(N, 2 * k)
        o = torch.zeros(self.n, dtype=torch.float32)
        for r in range(N):
            idx = rows[r, :k].long()
            o[idx] = o[idx] + rows[r, k:].view(torch.float32)
        return o / float(N) if N != 1 else o

    # ---- AdamW behind the decompressed average ---------------------------------------------------
    adam_grid = property(lambda self: (self.n + 2047) // 2048,
                         doc="workgroups of the update_adam launch (sizes the tickets)")

    def decay_runs(self, segments) -> torch.Tensor:
        """``int32[nr, 2] = (start, decays)`` on the core's device from ``segments`` of ``(offset,
        decays)``, one per tensor, offsets multiples of 16: sorted, the first run starting at 0 and
        neighbours that decay alike merged (a tensor's padding belongs to its run).  Built before any
        capture."""
        runs = []
        for off, dec in sorted((int(o), int(bool(d))) for o, d in segments):
            if off % 16 or not 0 <= off < self.n:
                raise ValueError(f"top-k: a tensor at offset {off} (multiples of 16 within n = {self.n} required)")
            if not runs or runs[-1][1] != dec:
                runs.append((off if runs else 0, dec))
        if not runs:
            raise ValueError("top-k: no segments")
        return torch.tensor(runs, dtype=torch.int32).to(self.device)

    def update_adam(self, x: torch.Tensor, m: torch.Tensor, v: torch.Tensor, gathered: torch.Tensor, lr: float,
                    wd: float, beta1: float, beta2: float, eps: float, block, decays: torch.Tensor,
                    hyper: Optional[torch.Tensor] = None) -> None:
        """Step 5 with AdamW (ops/adamw.py's rule, ``g := o``, ``div = 1``) behind the decompressed
        average ``o``: ``m`` / ``v`` the moments, ``block`` the :class:`ops.adamw.AdamState` (advanced
        once), ``decays`` from :meth:`decay_runs`.  ``hyper`` as for :meth:`update`."""
        self._check(x, m, v)
        N, k = self.world, self.k
        if gathered.dtype != torch.int32 or gathered.numel() != N * 2 * k or not gathered.is_contiguous():
            raise ValueError(f"TopKCore.update_adam: gathered must be contiguous int32 [{N}, {2 * k}]")
        if decays.dtype != torch.int32 or decays.dim() != 2 or decays.shape[1] != 2 or decays.device != self.device:
            raise ValueError(f"TopKCore.update_adam: decays must be int32 [runs, 2] on {self.device}")
        if self.device.type == "cuda":
            if hyper is None and wd != 0.0:
                raise ValueError("TopKCore.update_adam: weight decay on the device goes through the hyper block")
            ext().topk_update_adam(x, m, v, gathered, k, N, decays, float(lr), hyper, block.dev, block.ctr,
                                   float(beta1), float(beta2), float(eps))
            return
        o = self._decode(gathered)
        run = torch.bucketize(torch.arange(self.n), decays[:, 0].long().contiguous(), right=True) - 1
        dec = decays[run.clamp_(min=0), 1].bool()
        block.twin_step(x, m, v, [(dec, o[dec], True), (~dec, o[~dec], False)], lr, wd, beta1, beta2, eps)
