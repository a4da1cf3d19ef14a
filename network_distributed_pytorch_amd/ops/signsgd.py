"""Scaled-sign gradient compression with error feedback on gfx950 (csrc/signsgd.hip): EF-SignSGD,
the PowerSGD paper's "Sign+Norm".  One launch packs the signs of ``m = g + e`` (a wave ballot per 64
of them) and one fp32 magnitude per block of 2048 elements and leaves ``e = m - c``; one launch behind
the all-gather decompresses every rank's bits, averages and applies momentum SGD.

The rule (exact: bitwise identical on the device and in the torch twin that CPU tensors run), over
flat fp32 arenas of ``n`` elements ``g`` (gradient), ``e`` (error memory), ``x`` (weights), ``b``
(momentum).  Every segment ``(offset, numel)`` of the arena (a parameter; ``offset`` a multiple of
16) is cut into ``ceil(numel / G)`` blocks, ``G = 2048``; block ``j`` is ``(off_j, len_j)``,
``1 <= len_j <= G``, only a segment's last block is ragged.  Elements outside every block are
neither read nor written.  For block ``j`` and its in-block index ``t`` (``i = off_j + t``):

1. ``m_i = fadd(g_i, e_i)``.
2. ``S_j = sum |m_i|`` in fp64 in one fixed order, absent elements adding ``+0.0``: with
   ``t = 1024 h + 256 w + 4 l + c`` (round ``h`` < 2, wave ``w`` < 4, lane ``l`` < 64, component
   ``c`` < 4), per (w, l): ``s = 0; for h: for c: s += |m|``; per w the butterfly
   ``for o in 32, 16, 8, 4, 2, 1: s_l += s_(l ^ o)``; then ``S = ((s_0 + s_1) + s_2) + s_3``.
3. ``s_j = (float)(S_j / (double)len_j)``: IEEE fp64 division, one rounding to fp32.  NaN / inf in
   the block make it NaN / inf; it is sent and reaches every replica.
4. ``c_i`` = the float with the bits ``(bits(s_j) & 0x7fffffff) | (bits(m_i) & 0x80000000)``
   (``-0`` sends bit 1).
5. ``e_i' = fsub(m_i, c_i)``.
6. Wire buffer ``int32[nb * 65]``: ``nb * 64`` sign words, then ``nb`` words ``bits(s_j)``.  The
   sign of the in-block element ``t`` of block ``j`` is bit ``bit(t)`` of word ``word(t)``::

       word(t) = 64 j + 8 (t >> 8) + 2 (t & 3) + ((t >> 7) & 1),      bit(t) = (t >> 2) & 31

   (the 64-bit ballot of wave ``w``, round ``h``, component ``c`` is the little-endian word pair
   number ``16 h + 4 w + c`` of the block).  Bits of absent elements are 0.
7. The ranks' buffers are gathered into ``[N, nb * 65]`` (one all-gather; none with ``N = 1``).
8. Per element ``acc = 0``; for ``r = 0 .. N-1`` in rank order ``acc = fadd(acc, c_{r,i})``;
   ``o = acc / N`` when ``N != 1`` else ``acc``; then the element rule of the other arms:
   ``d = (wd != 0) ? fmaf(wd, x, o) : o``; ``b' = fadd(fmul(b, lambda), d)``; ``up = fadd(d, b')``;
   ``x' = fmaf(-lr, up, x)``.

Device tensors run the native kernels, CPU tensors the twin; a device tensor the kernels cannot
take (not fp32, not contiguous) is an error, never a fallback.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from ._ext import ext
from .topk import fmaf32

__all__ = ["SignCore", "sign_word_bit"]

G = 2048  # elements per block: csrc/ndp_kernels.h kSignBlock
_MAG, _SIGN = 0x7FFFFFFF, -0x80000000


def sign_word_bit(j, t):
    """``(word, bit)`` of in-block element ``t`` of block ``j`` in the sign words of a wire buffer."""
    return 64 * j + 8 * (t >> 8) + 2 * (t & 3) + ((t >> 7) & 1), (t >> 2) & 31


class SignCore:
    """Block table, output and gathered buffers of one scaled-sign compressor over arenas of ``n``
    elements whose live parts are ``segments = [(offset, numel), ...]``; everything is allocated
    (and the table uploaded) here, before any capture.  ``out`` is this rank's ``int32[nb * 65]``,
    ``gathered`` the ``[world, nb * 65]`` the update reads (``out`` itself when ``world == 1``)."""

    block = G

    def __init__(self, device, segments: Sequence[Tuple[int, int]], n: int, world: int = 1):
        self.device = torch.device(device)
        self.n, self.world = int(n), int(world)
        if not 1 <= self.n < 2 ** 31:
            raise ValueError(f"signsgd: 1 <= n < 2^31 required, got n = {n}")
        if self.world < 1:
            raise ValueError(f"signsgd: world >= 1 required, got {world}")
        table, end = [], 0
        self._block_seg = []  # per block, the position of its segment in `segments` as given
        for off, numel, s in sorted((int(o), int(c), s) for s, (o, c) in enumerate(segments)):
            if off % 16 or numel < 1 or off < end or off + numel > self.n:
                raise ValueError(f"signsgd: segment ({off}, {numel}) must start at a multiple of 16, be non-empty, "
                                 f"follow the segment before it (which ends at {end}) and end within n = {self.n}")
            table += [(off + t, min(G, numel - t)) for t in range(0, numel, G)]
            self._block_seg += [s] * ((numel + G - 1) // G)
            end = off + numel
        if not table:
            raise ValueError("signsgd: no segments")
        self.nb, self.words = len(table), len(table) * (G // 32 + 1)
        self._host_table = torch.tensor(table, dtype=torch.int32)
        i32 = dict(dtype=torch.int32, device=self.device)
        self.out = torch.zeros(self.words, **i32)
        self.gathered = self.out.view(1, -1) if self.world == 1 else torch.zeros(self.world, self.words, **i32)
        self.table = self._twin = None
        if self.device.type == "cuda":
            assert not torch.cuda.is_current_stream_capturing(), "SignCore is built before capture"
            self.table = self._host_table.to(self.device)

    def _check(self, *tensors):
        for t in tensors:
            if t.device != self.device:
                raise ValueError(f"SignCore on {self.device}: tensor on {t.device}")
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != self.n:
                raise ValueError(f"SignCore: arenas must be contiguous float32 of {self.n} elements "
                                 f"(got {t.dtype}, contiguous={t.is_contiguous()}, numel={t.numel()})")

    def _twin_index(self):
        """``idx`` [nb, G] arena index of every (block, t), clamped into the block where absent, and
        ``valid`` [nb, G]."""
        if self._twin is None:
            off, ln = self._host_table[:, :1].long(), self._host_table[:, 1:].long()
            t = torch.arange(G).view(1, G)
            self._twin = (off + torch.minimum(t, ln - 1), t < ln)
        return self._twin

    def compress(self, g: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
        """Steps 1-6: ``e`` becomes the residual, ``out`` the wire buffer; returns ``out``."""
        self._check(g, e)
        if self.device.type == "cuda":
            ext().sign_pack(g, e, self.table, self.nb, self.out)
            return self.out
        nb, (idx, valid) = self.nb, self._twin_index()
        m = torch.where(valid, g[idx] + e[idx], torch.zeros(()))
        mb = m.view(torch.int32)
        a = m.abs().double().view(nb, 2, 4, 64, 4)  # [block, h, w, lane, c]
        s = a[:, 0, :, :, 0]  # 0 + a is a
        for h, c in [(0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3)]:
            s = s + a[:, h, :, :, c]
        lane = torch.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, :, lane ^ o]
        S = ((s[:, 0, 0] + s[:, 1, 0]) + s[:, 2, 0]) + s[:, 3, 0]
        sc = (S / self._host_table[:, 1].double()).float()
        # signs: [block, h, w, lane, c] -> [block, h, w, c, lane] = 32 ballots of 64 bits, low word first
        bit = ((mb >> 31) & 1).view(nb, 2, 4, 64, 4).permute(0, 1, 2, 4, 3).reshape(nb, 64, 32).long()
        words = (bit << torch.arange(32)).sum(-1)  # < 2^32, wrapped into int32 below
        self.out[: nb * 64] = ((words + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32).view(-1)
        self.out[nb * 64:] = sc.view(torch.int32)
        c = ((sc.view(torch.int32) & _MAG).view(nb, 1) | (mb & _SIGN)).view(torch.float32)
        # m - c as m + (-c): the same float wherever c is a number.  Where it is NaN this gives the
        # NaN gfx950's subtraction returns: m itself if m is NaN, else c with its sign flipped (the
        # host's subtraction would keep that sign)
        e[idx[valid]] = torch.where(torch.isnan(m), m, m + c.neg())[valid]
        return self.out

    def update(self, x: torch.Tensor, b: torch.Tensor, gathered: torch.Tensor, lr: float, lam: float,
               wd: float = 0.0, hyper: Optional[torch.Tensor] = None) -> None:
        """Step 8 over ``gathered`` (``int32 [world, nb * 65]``).  On a device ``lr`` goes by value and
        there is no decay unless ``hyper``, the block ``[lr, weight_decay, 0, 0]``, is given (then
        ``lr`` / ``wd`` here are ignored)."""
        self._check(x, b)
        N, nb = self.world, self.nb
        if gathered.dtype != torch.int32 or gathered.numel() != N * self.words or not gathered.is_contiguous():
            raise ValueError(f"SignCore.update: gathered must be contiguous int32 [{N}, {self.words}]")
        if self.device.type == "cuda":
            if hyper is None and wd != 0.0:
                raise ValueError("SignCore.update: weight decay on the device goes through the hyper block")
            ext().sign_update(x, b, self.table, nb, gathered, N, float(lr), float(lam), hyper)
            return
        idx, valid = self._twin_index()
        o = self._decode(gathered)
        lr, lam, wd = (float(np.float32(v)) for v in (lr, lam, wd))
        xv, bv = x[idx], b[idx]
        d = fmaf32(wd, xv, o) if wd != 0 else o
        bv = bv * lam + d
        xv = fmaf32(-lr, d + bv, xv)
        x[idx[valid]], b[idx[valid]] = xv[valid], bv[valid]

    def _decode(self, gathered: torch.Tensor) -> torch.Tensor:
        """The twin's ``o`` of step 8, ``[nb, G]``: the rank-ordered sum of the ``c_r``, over ``N``."""
        N, nb = self.world, self.nb
        rows = gathered.view(N, self.words)
        o = torch.zeros(nb, G)
        for r in range(N):
            words = rows[r, : nb * 64].view(nb, 64, 1)
            bit = ((words >> torch.arange(32, dtype=torch.int32)) & 1).view(nb, 2, 4, 4, 64)  # [block, h, w, c, lane]
            bit = bit.permute(0, 1, 2, 4, 3).reshape(nb, G)
            mag = (rows[r, nb * 64:] & _MAG).view(nb, 1)
            o = o + (mag | (bit * _SIGN)).view(torch.float32)
        return o / float(N) if N != 1 else o

    # ---- AdamW behind the decompressed average ---------------------------------------------------
    adam_grid = property(lambda self: self.nb, doc="workgroups of the update_adam launch (sizes the tickets)")

    def block_decays(self, flags: Sequence[bool]) -> torch.Tensor:
        """``int32[nb]`` on the core's device: per block, whether its tensor takes the weight decay;
        ``flags`` one per segment, in the order the segments were given.  Built before any capture."""
        flags = [bool(f) for f in flags]
        if len(flags) != max(self._block_seg) + 1:
            raise ValueError(f"{type(self).__name__}: {len(flags)} decay flags for {max(self._block_seg) + 1} segments")
        return torch.tensor([int(flags[s]) for s in self._block_seg], dtype=torch.int32).to(self.device)

    def _native_update_adam(self, x, m, v, gathered, lr, hyper, block, decays, beta1, beta2, eps):
        ext().sign_update_adam(x, m, v, self.table, decays, self.nb, gathered, self.world, float(lr), hyper,
                               block.dev, block.ctr, float(beta1), float(beta2), float(eps))

    def update_adam(self, x: torch.Tensor, m: torch.Tensor, v: torch.Tensor, gathered: torch.Tensor, lr: float,
                    wd: float, beta1: float, beta2: float, eps: float, block, decays: torch.Tensor,
                    hyper: Optional[torch.Tensor] = None) -> None:
        """The update with AdamW (ops/adamw.py's rule, ``g := o``, ``div = 1``) behind the decompressed
        average ``o``: ``m`` / ``v`` the moments, ``block`` the :class:`ops.adamw.AdamState` (advanced
        once), ``decays`` from :meth:`block_decays`.  ``hyper`` as for :meth:`update`."""
        self._check(x, m, v)
        if gathered.dtype != torch.int32 or gathered.numel() != self.world * self.words or not gathered.is_contiguous():
            raise ValueError(f"{type(self).__name__}.update_adam: gathered must be contiguous int32 "
                             f"[{self.world}, {self.words}]")
        if decays.dtype != torch.int32 or decays.numel() != self.nb or decays.device != self.device:
            raise ValueError(f"{type(self).__name__}.update_adam: decays must be int32 [{self.nb}] on {self.device}")
        if self.device.type == "cuda":
            if hyper is None and wd != 0.0:
                raise ValueError(f"{type(self).__name__}.update_adam: weight decay on the device goes through the "
                                 f"hyper block")
            self._native_update_adam(x, m, v, gathered, lr, hyper, block, decays, beta1, beta2, eps)
            return
        idx, valid = self._twin_index()
        o = self._decode(gathered)
        dec = decays.bool().view(-1, 1)
        block.twin_step(x, m, v, [(idx[valid & dec], o[valid & dec], True), (idx[valid & ~dec], o[valid & ~dec], False)],
                        lr, wd, beta1, beta2, eps)
