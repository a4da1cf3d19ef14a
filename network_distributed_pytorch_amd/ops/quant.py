"""Block-quantised gradient compression with error feedback on gfx950 (csrc/quant.hip): fixed-point
codes of 2, 4 or 8 bits with one fp32 scale per block (QSGD / TernGrad style with deterministic
rounding; at 2 bits the code is ternary).  One launch quantises ``m = g + e`` against each block's
absmax and leaves ``e = m - c``; one launch behind the all-gather decodes every rank's codes, averages
and applies momentum SGD.  Dense is 4 bytes per element; this sends ``bits / 8`` plus 4 bytes per block.

The rule (exact: bitwise identical on the device and in the torch twin that CPU tensors run, on finite
inputs), over the arenas and the blocks of ops/signsgd.py: every segment ``(offset, numel)`` is cut
into blocks of ``G = 2048``, block ``j`` is ``(off_j, len_j)``, only a segment's last block is ragged,
elements outside every block are neither read nor written.  With ``b = bits``, ``L = 2^(b-1) - 1``
(1, 7, 127) and ``t`` the in-block index:

1. ``m = fadd(g, e)``.
2. ``A_j = max(bits(m) & 0x7fffffff)`` as unsigned integers: the exact absmax, whatever the order.
3. ``s_j = fdiv(A_j, (float)L)``.  The block is *finite* when ``A_j < 0x7f800000`` and *dead* when
   ``s_j == 0`` (a zero block, or underflow).
4. Finite, live block: ``q = clamp(rint(fdiv(m, s_j)), -L, L)``, round half to even, kept as a float
   (so ``rint(-0.3) = -0`` stays ``-0``); ``c = fmul(q, s_j)``; ``e' = fsub(m, c)``; the stored code is
   ``u = (int)q + L``.  The rounding is deterministic: the error feedback absorbs its bias.
5. Dead block: every code bit 0, scale word 0, ``e' = m``.  Non-finite block: every code bit 0, scale
   word ``0x7fc00000``, every ``e'`` the bit pattern ``0x7fc00000``; the update then gives NaN weights
   for the block on every replica.
6. Row of a rank, ``int32[row_words]``: ``nb * W`` code words (``W = 64 b``), ``nb`` scale words
   ``bits(s_j)``, zero padding up to a multiple of 4 words (rows of the gathered buffer stay 16-byte
   aligned).  The codes of block ``j`` are a little-endian bit stream: element ``t`` is the bits
   ``[(t b) & 31, +b)`` of word ``W j + ((t b) >> 5)`` (:func:`quant_word_shift`).  Bits of absent
   elements are 0.
7. Per element ``acc = 0``; for ``r = 0 .. N-1`` in rank order
   ``acc = fadd(acc, fmul((float)(u_r - L), s_{r,j}))``; ``o = acc / N`` when ``N != 1``; then the
   element rule of the other arms: ``d = (wd != 0) ? fmaf(wd, x, o) : o``;
   ``b' = fadd(fmul(b, lambda), d)``; ``x' = fmaf(-lr, fadd(d, b'), x)``.

Randomized Hadamard rotation (``rotate="hadamard"``; DRIVE / EDEN of Vargaftik et al. 2021/22): one
large coordinate sets a block's absmax and the rest of the block rounds to zero; behind ``y = W (d o m)``
the coordinates are near-Gaussian whatever the block looked like.  A block is *rotated* iff
``len_j == 2048``; a ragged block follows the rule above unchanged.  The wire row does not change by a
bit.  For a rotated block:

* Signs: ``d_t = -1`` iff bit ``t & 31`` of ``hash4(rotate_seed, j, t >> 5, 0x48414452)`` is set
  (:func:`quant_rotate_signs`); applying ``d_t`` flips the float's sign bit.
* ``W`` (:func:`quant_fwht`): 11 butterfly stages ``k = 0 .. 10`` in that order; in stage ``k`` every pair
  ``(t, t | 2^k)`` with bit ``k`` of ``t`` clear becomes ``(fadd(a, b), fsub(a, b))``, each one IEEE fp32
  operation.  It is the natural-order Sylvester Hadamard matrix ``H[t][u] = (-1)^popcount(t & u)``,
  unnormalised: ``W(W(v)) = 2048 v``.
* Step 1 becomes ``m = fadd(W(d o g), e)``: the error memory of a rotated block lives in the rotated
  domain.  Steps 2 to 6 run on this ``m`` unchanged; an overflow inside the butterflies makes the block
  non-finite like an inf in ``g``.
* Step 7 forms ``acc`` as above (in the rotated domain), then ``a_t = d_t fmul(W(acc)_t, 2^-11)`` (one
  transform per block, not per rank: ``W`` is linear) and goes on with ``a`` in the place of ``acc``.

Device tensors run the native kernels, CPU tensors the twin; a device tensor the kernels cannot
take (not fp32, not contiguous) is an error, never a fallback.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from ._ext import ext
from .image_batch import _hash4_t
from .signsgd import G, SignCore
from .topk import fmaf32

__all__ = ["QuantCore", "quant_word_shift", "quant_fwht", "quant_rotate_signs", "QUANT_BITS", "QUANT_ROTATIONS"]

QUANT_BITS = (2, 4, 8)
QUANT_ROTATIONS = ("none", "hadamard")
_ROT_TAG = 0x48414452  # csrc/quant.hip kRotTag
_MAG, _INF, _NAN = 0x7FFFFFFF, 0x7F800000, 0x7FC00000


def quant_word_shift(bits, j, t):
    """``(word, shift)`` of the code of in-block element ``t`` of block ``j`` in a row."""
    return 64 * bits * j + ((t * bits) >> 5), (t * bits) & 31


def quant_fwht(v: torch.Tensor) -> torch.Tensor:
    """``W`` over the last dimension (2048) of an fp32 tensor: the 11 stages in the rule's order."""
    shape = v.shape
    for k in range(11):
        v = v.reshape(-1, G >> (k + 1), 2, 1 << k)
        a, b = v[:, :, 0], v[:, :, 1]
        v = torch.stack((a + b, a - b), dim=2)
    return v.reshape(shape)


def quant_rotate_signs(seed: int, j: int) -> torch.Tensor:
    """``d`` of block ``j`` as fp32 ``[2048]`` of ``+1`` / ``-1`` (a product with it flips the sign bit)."""
    words = _hash4_t(seed, j, torch.arange(G // 32), _ROT_TAG).view(-1, 1)
    return (1 - 2 * ((words >> torch.arange(32)) & 1)).view(G).float()


class QuantCore(SignCore):
    """:class:`SignCore`'s block table and interface with rows of ``words = row_words`` int32:
    ``out`` is this rank's row, ``gathered`` the ``[world, words]`` the update reads (``out`` itself
    when ``world == 1``); everything is allocated here, before any capture."""

    def __init__(self, device, segments: Sequence[Tuple[int, int]], n: int, world: int = 1, bits: int = 4,
                 rotate: str = "none", rotate_seed: int = 0):
        if bits not in QUANT_BITS:
            raise ValueError(f"quant: bits must be one of {QUANT_BITS}, got {bits!r}")
        if rotate not in QUANT_ROTATIONS:
            raise ValueError(f"quant: rotate must be one of {QUANT_ROTATIONS}, got {rotate!r}")
        if not 0 <= int(rotate_seed) < 2 ** 32:
            raise ValueError(f"quant: 0 <= rotate_seed < 2^32 required, got {rotate_seed!r}")
        super().__init__(device, segments, n, world)
        self.rotate, self.rotate_seed, self._rot = rotate, int(rotate_seed), None
        self.bits, self.levels = int(bits), 2 ** (int(bits) - 1) - 1
        self.code_words = 64 * self.bits * self.nb
        self.words = (self.code_words + self.nb + 3) // 4 * 4
        i32 = dict(dtype=torch.int32, device=self.device)
        self.out = torch.zeros(self.words, **i32)
        self.gathered = self.out.view(1, -1) if self.world == 1 else torch.zeros(self.world, self.words, **i32)

    def _twin_rotation(self):
        """``(rotated [nb, 1] bool, d [nb, G])`` of the twin; ``d`` is 1 in the blocks that are not rotated."""
        if self._rot is None:
            rotated = (self._host_table[:, 1:] == G) & (self.rotate == "hadamard")
            d = torch.ones(self.nb, G)
            for j in rotated.view(-1).nonzero().view(-1).tolist():
                d[j] = quant_rotate_signs(self.rotate_seed, j)
            self._rot = (rotated, d)
        return self._rot

    def compress(self, g: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
        """Steps 1-6: ``e`` becomes the residual, ``out`` the row; returns ``out``."""
        self._check(g, e)
        nb, bits, L = self.nb, self.bits, self.levels
        if self.device.type == "cuda":
            ext().quant_pack(g, e, self.table, nb, bits, self.out, self.rotate, self.rotate_seed)
            return self.out
        idx, valid = self._twin_index()
        y = g[idx]
        if self.rotate != "none":
            rotated, d = self._twin_rotation()
            y = torch.where(rotated, quant_fwht(y * d), y)
        m = torch.where(valid, y + e[idx], torch.zeros(()))
        A = (m.view(torch.int32) & _MAG).max(dim=1, keepdim=True).values
        s = A.view(torch.float32) / float(L)
        finite = A < _INF
        live = finite & (s != 0)
        q = torch.round(m / s).clamp(-float(L), float(L))
        u = torch.where(valid & live, torch.nan_to_num(q).long() + L, torch.zeros((), dtype=torch.long))
        words = (u.view(nb, 64 * bits, 32 // bits) << (torch.arange(32 // bits) * bits)).sum(-1)  # < 2^32
        self.out.zero_()
        self.out[: self.code_words] = ((words + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32).view(-1)
        scale = torch.where(live, s.view(torch.int32), torch.where(finite, 0, _NAN))
        self.out[self.code_words: self.code_words + nb] = scale.view(-1).to(torch.int32)
        nan = torch.full((), _NAN, dtype=torch.int32).view(torch.float32)
        e[idx[valid]] = torch.where(live, m - q * s, torch.where(finite, m, nan))[valid]
        return self.out

    def update(self, x: torch.Tensor, b: torch.Tensor, gathered: torch.Tensor, lr: float, lam: float,
               wd: float = 0.0, hyper: Optional[torch.Tensor] = None) -> None:
        """Step 7 over ``gathered`` (``int32 [world, words]``).  On a device ``lr`` goes by value and
        there is no decay unless ``hyper``, the block ``[lr, weight_decay, 0, 0]``, is given (then
        ``lr`` / ``wd`` here are ignored)."""
        self._check(x, b)
        N, nb, bits = self.world, self.nb, self.bits
        if gathered.dtype != torch.int32 or gathered.numel() != N * self.words or not gathered.is_contiguous():
            raise ValueError(f"QuantCore.update: gathered must be contiguous int32 [{N}, {self.words}]")
        if self.device.type == "cuda":
            if hyper is None and wd != 0.0:
                raise ValueError("QuantCore.update: weight decay on the device goes through the hyper block")
            ext().quant_update(x, b, self.table, nb, bits, gathered, N, float(lr), float(lam), hyper, self.rotate,
                               self.rotate_seed)
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
        """The twin's ``o`` of step 7, ``[nb, G]``: the rank-ordered sum of the decoded codes (rotated back
        where the block is rotated), over ``N``."""
        N, nb, bits = self.world, self.nb, self.bits
        rows = gathered.view(N, self.words)
        shifts = (torch.arange(32 // bits) * bits).to(torch.int32)
        o = torch.zeros(nb, G)
        for r in range(N):
            u = ((rows[r, : self.code_words].view(nb, 64 * bits, 1) >> shifts) & (2 ** bits - 1)).view(nb, G)
            scale = rows[r, self.code_words: self.code_words + nb].view(torch.float32).view(nb, 1)
            o = o + (u - self.levels).float() * scale
        if self.rotate != "none":
            rotated, d = self._twin_rotation()
            o = torch.where(rotated, d * (quant_fwht(o) * 2.0 ** -11), o)
        return o / float(N) if N != 1 else o

    def _native_update_adam(self, x, m, v, gathered, lr, hyper, block, decays, beta1, beta2, eps):
        ext().quant_update_adam(x, m, v, self.table, decays, self.nb, self.bits, gathered, self.world, float(lr), hyper,
                                block.dev, block.ctr, float(beta1), float(beta2), float(eps), self.rotate,
                                self.rotate_seed)
