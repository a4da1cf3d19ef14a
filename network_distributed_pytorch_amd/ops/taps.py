"""Which taps of a conv weight can ever receive gradient ("live" taps).

On a small feature map most taps of a padded kernel only ever multiply padding: a 3x3, pad-1
conv on a 1x1 map reads real pixels through its centre tap alone.  The gradient of the other
taps is exactly zero on every step, so (without weight decay) their error memory and momentum
stay zero for ever.  ``GemmConv2d`` records, on the weight Parameter itself, the union of the
live taps of every input size it trains on; the PowerSGD optimizer keeps the error memory and
momentum of such a weight compact — ``[n, live columns]`` — and skips the dead columns' HBM
traffic (csrc/plan.cpp, csrc/powersgd.hip).

The column maps here are the host mirror of ``MatGeom``'s (csrc/plan.h): a weight
``[Co, C, KH, KW]`` viewed as ``[Co, C * T]`` with tap period ``T = KH * KW`` and ``L`` live
taps has compact column ``j`` at full column ``(j // L) * T + tap[j % L]``.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

__all__ = ["live_taps", "mark", "record", "version", "support_of", "tap_list", "full_cols", "compact_col", "compact_cols", "expand",
           "compress", "dead_all_zero", "MAX_PERIOD"]

MAX_PERIOD = 16  # csrc/ndp_kernels.h kMaxTapPeriod: the packed tap list holds 16 taps
_ATTR = "_ndp_taps"
_VERSION = 0


def _pair(v) -> Tuple[int, int]:
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def _live_1d(size: int, k: int, stride: int, pad: int) -> List[bool]:
    out = (size + 2 * pad - k) // stride + 1
    return [any(0 <= o * stride - pad + t < size for o in range(out)) for t in range(k)]


def live_taps(H: int, W: int, KH: int, KW: int, stride, pad) -> int:
    """Bitmask over ``KH * KW`` (bit ``kh * KW + kw``): the taps through which some output
    position of a zero-padded, undilated conv on an ``H x W`` map reads a real pixel."""
    (sh, sw), (ph, pw) = _pair(stride), _pair(pad)
    rows, cols = _live_1d(H, KH, sh, ph), _live_1d(W, KW, sw, pw)
    mask = 0
    for kh in range(KH):
        for kw in range(KW):
            if rows[kh] and cols[kw]:
                mask |= 1 << (kh * KW + kw)
    return mask


def version() -> int:
    """Process-wide counter, bumped whenever some weight's recorded support widens."""
    return _VERSION


def mark(weight: torch.Tensor, T: int, mask: int) -> None:
    """Widen ``weight``'s recorded support (tap period ``T``) by the taps of ``mask``."""
    global _VERSION
    old = getattr(weight, _ATTR, None)
    new = mask if old is None else (old[1] | mask)
    if old is None or new != old[1]:
        setattr(weight, _ATTR, (T, new))
        _VERSION += 1


def record(weight: torch.Tensor, H: int, W: int, stride, pad) -> None:
    """Widen ``weight``'s recorded support by the live taps of an ``H x W`` input."""
    KH, KW = int(weight.shape[-2]), int(weight.shape[-1])
    mark(weight, KH * KW, live_taps(H, W, KH, KW, stride, pad))


def support_of(p: torch.Tensor) -> Optional[Tuple[int, int]]:
    """``(T, mask)`` recorded on a parameter, or None (never seen by a recording conv)."""
    return getattr(p, _ATTR, None)


def tap_list(T: int, mask: int) -> List[int]:
    return [t for t in range(T) if mask >> t & 1]


def compact_cols(m: int, T: int, mask: int) -> int:
    return (m // T) * len(tap_list(T, mask))


def full_cols(m: int, T: int, mask: int) -> torch.Tensor:
    """Full column of every compact column (int64, ``[(m // T) * L]``)."""
    taps = torch.tensor(tap_list(T, mask), dtype=torch.int64)
    return (torch.arange(m // T, dtype=torch.int64)[:, None] * T + taps[None, :]).reshape(-1)


def compact_col(b: int, T: int, mask: int) -> int:
    """Inverse of :func:`full_cols`: compact column of full column ``b`` (-1: dead tap)."""
    t = b % T
    if not mask >> t & 1:
        return -1
    return (b // T) * len(tap_list(T, mask)) + bin(mask & ((1 << t) - 1)).count("1")


def compress(full: torch.Tensor, T: int, mask: int) -> torch.Tensor:
    """``[n, m]`` full layout -> ``[n, live columns]``."""
    n, m = full.shape
    return full.reshape(n, m // T, T)[:, :, tap_list(T, mask)].reshape(n, -1)


def expand(compact: torch.Tensor, m: int, T: int, mask: int) -> torch.Tensor:
    """``[n, live columns]`` -> ``[n, m]`` full layout, zeros in the dead columns."""
    n = compact.shape[0]
    taps = tap_list(T, mask)
    out = compact.new_zeros(n, m // T, T)
    out[:, :, taps] = compact.reshape(n, m // T, len(taps))
    return out.reshape(n, m)


def dead_all_zero(full: torch.Tensor, T: int, mask: int) -> bool:
    """Whether every dead-tap entry of a full-layout ``[n, m]`` matrix is zero (host sync)."""
    n, m = full.shape
    dead = [t for t in range(T) if not mask >> t & 1]
    if not dead:
        return True
    return not bool(full.reshape(n, m // T, T)[:, :, dead].any().item())
