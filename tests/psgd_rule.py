"""Test-only stage rules of the PowerSGD reducer, per matrix, written from the README's element rule
and the MatGeom comment of csrc/ndp_kernels.h.  Plain torch on the CPU, no framework code.

Inputs are fp32 tensors.  Every reduction (P = M Q, Q = M^T P-hat, out = P-hat Qs^T) is one fp64
matmul of the fp32 operands; every op of the element chain is computed in fp64 from operands that
are fp32 values and rounded once to fp32 (``_r``).  The results are fp64 tensors that hold fp32
values wherever the chain ends in a rounding; a reduction's result is left in fp64.

``absolute=True`` evaluates the same rule with every input replaced by its absolute value and every
subtraction by an addition, without rounding: the magnitude S of the derived error bound
``|dev - ref| <= (K + 8) * 2^-24 * S`` (K: fp32 operations of the longest path).

The three input arms (``arm_inputs``) make the rule exact in two cases and bounded in the third:
  int       small integers: every product and every sum is exact in fp32 in any order;
  mantissa  full 24-bit mantissas on the streamed operand, a one-nonzero +-2^k selector as the small
            operand and power-of-two constants: every output is one exact product or a chain of
            single correctly rounded ops;
  normal    seeded Gaussians, compared within the bound above.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

ARMS = ("int", "mantissa", "normal")
EPS32 = 2.0 ** -24


def _r(t: torch.Tensor) -> torch.Tensor:
    """one rounding to fp32, kept in fp64"""
    return t.float().double()


class _Ops:
    def __init__(self, absolute: bool):
        self.absolute = absolute

    def inp(self, t):
        t = t.double()
        return t.abs() if self.absolute else t

    def rnd(self, t):
        return t if self.absolute else _r(t)

    def sub(self, a, b):
        return self.rnd(a + b if self.absolute else a - b)

    def add(self, a, b):
        return self.rnd(a + b)

    def mul(self, a, s: float):
        return self.rnd(a * (abs(s) if self.absolute else s))

    def fma(self, s: float, a, b):  # s a + b, one rounding
        return self.rnd((abs(s) if self.absolute else s) * a + b)


# ---- dead-tap layout (MatGeom tap_*): compact column j is full column (j // L) * T + tap[j % L] ----
def live_taps(T: int, mask: int) -> List[int]:
    return [t for t in range(T) if mask >> t & 1]


def full_columns(m: int, T: int, mask: int) -> torch.Tensor:
    taps = live_taps(T, mask)
    L = len(taps)
    assert m % T == 0 and 1 <= L < T
    return torch.tensor([(j // L) * T + taps[j % L] for j in range((m // T) * L)], dtype=torch.long)


def compress(full: torch.Tensor, T: int, mask: int) -> torch.Tensor:
    """[n, m] -> [n, (m / T) L]"""
    return full[:, full_columns(full.shape[1], T, mask)].contiguous()


def expand(compact: torch.Tensor, m: int, T: int, mask: int, fill: float = 0.0) -> torch.Tensor:
    """[n, (m / T) L] -> [n, m], the dead columns ``fill``"""
    out = torch.full((compact.shape[0], m), fill, dtype=compact.dtype)
    out[:, full_columns(m, T, mask)] = compact
    return out


# ---- stages --------------------------------------------------------------------------------------
def p_stage(g, Q, e=None, p_prev=None, absolute=False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """P = M Q with M = g + e_eff.  e None: fuse_ef off (M = g, nothing stored).  p_prev given:
    e_eff = e - P_prev Q^T (Q is the previous update's Qs).  Returns (P, M or None); M is what the
    e slot holds afterwards."""
    o = _Ops(absolute)
    g, Q = o.inp(g), o.inp(Q)
    if e is None:
        assert p_prev is None
        return g @ Q, None
    e = o.inp(e)
    if p_prev is not None:
        e = o.sub(e, o.rnd(o.inp(p_prev) @ Q.t()))
    M = o.add(g, e)
    return M @ Q, M


def q_stage(M, P_hat, absolute=False) -> torch.Tensor:
    o = _Ops(absolute)
    return o.inp(M).t() @ o.inp(P_hat)


def element_step(o: _Ops, out, mom, x, lr, momentum, wd):
    """README element rule -> (d, m', up, x')"""
    d = o.fma(wd, x, out) if wd != 0 else out
    mm = o.add(o.mul(mom, momentum), d)
    up = o.add(d, mm)
    xx = o.rnd(x + abs(lr) * up) if o.absolute else o.fma(-lr, up, x)
    return d, mm, up, xx


def update_stage(mode: int, P_hat, Q_sum, q_div: float, M=None, mom=None, x=None, lr=0.0, momentum=0.0,
                 wd=0.0, lazy=False, absolute=False) -> Dict[str, torch.Tensor]:
    """Every array the update stage writes.  ``q_warm`` always; mode 0: out, mem; mode 3: e; modes 1 / 2:
    mom, x, (g with mode 2), and e when not lazy or p_prev when lazy."""
    o = _Ops(absolute)
    P_hat, Q_sum = o.inp(P_hat), o.inp(Q_sum)
    Qs = o.rnd(Q_sum / q_div)
    out = o.rnd(P_hat @ Qs.t())
    res = {"q_warm": Qs}
    if mode == 0:
        res["out"] = out
        res["mem"] = o.sub(o.inp(M), out)
        return res
    if mode == 3:
        res["e"] = o.sub(o.inp(M), out)
        return res
    assert mode in (1, 2)
    _, mm, up, xx = element_step(o, out, o.inp(mom), o.inp(x), lr, momentum, wd)
    res["mom"], res["x"] = mm, xx
    if mode == 2:
        res["g"] = up
    if lazy:
        res["p_prev"] = P_hat
    else:
        res["e"] = o.sub(o.inp(M), out)
    return res


def rank1_step(buf, div: float, mom, x, lr, momentum, wd=0.0, absolute=False) -> Dict[str, torch.Tensor]:
    o = _Ops(absolute)
    out = o.rnd(o.inp(buf) / div)
    _, mm, up, xx = element_step(o, out, o.inp(mom), o.inp(x), lr, momentum, wd)
    return {"mom": mm, "x": xx, "g": up}


def k_ops(stage: str, n: int, m: int, r: int) -> int:
    """fp32 operations of the longest path of one output element"""
    return {"p": m + r + 2, "q": n, "u": r + 6, "r1": 6}[stage]


# ---- input arms ----------------------------------------------------------------------------------
def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def _mant(gen, shape):
    """random sign, full 24-bit mantissa, exponent in [-4, 4]"""
    mant = torch.randint(1 << 23, 1 << 24, shape, generator=gen).double()
    ex = torch.randint(-4, 5, shape, generator=gen).double()
    sign = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
    v = sign * mant * torch.pow(torch.tensor(2.0, dtype=torch.float64), ex - 23)
    assert torch.equal(v.float().double(), v)
    return v.float()


def _pow2(gen, shape):
    ex = torch.randint(-2, 3, shape, generator=gen).double()
    sign = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
    return (sign * torch.pow(torch.tensor(2.0, dtype=torch.float64), ex)).float()


def selector_positions(gen, length: int, count: int, chunk: int) -> List[int]:
    """``count`` distinct positions in [0, length): 0, the last one, one inside the last partial
    chunk of ``chunk``, then random ones (count <= length)"""
    assert count <= length
    tail0 = ((length - 1) // chunk) * chunk
    want = [0, length - 1, tail0 + (length - 1 - tail0) // 2]
    pos: List[int] = []
    for p in want:
        if p not in pos and len(pos) < count:
            pos.append(p)
    perm = torch.randperm(length, generator=gen).tolist()
    for p in perm:
        if len(pos) == count:
            break
        if p not in pos:
            pos.append(p)
    return pos


def stream(arm: str, gen, shape, lim: int = 3) -> torch.Tensor:
    """an operand that is streamed from memory (g, e, M, mom, x, Q_sum, the rank-1 payload)"""
    if arm == "int":
        return _ints(gen, shape, -lim, lim)
    if arm == "mantissa":
        return _mant(gen, shape)
    return torch.randn(shape, generator=gen)


def small_q(arm: str, gen, m: int, r: int, chunk: int) -> torch.Tensor:
    """the P stage's Q [m, r]: mantissa arm: one nonzero row per column, rows distinct"""
    if arm == "int":
        return _ints(gen, (m, r), -2, 2)
    if arm == "normal":
        return torch.randn((m, r), generator=gen)
    Q = torch.zeros(m, r)
    Q[selector_positions(gen, m, r, chunk), torch.arange(r)] = _pow2(gen, (r,))
    return Q


def small_p_cols(arm: str, gen, n: int, r: int, chunk: int) -> torch.Tensor:
    """the Q stage's P-hat [n, r]: mantissa arm: one nonzero row per column"""
    return small_q(arm, gen, n, r, chunk)


def small_p_rows(arm: str, gen, n: int, r: int) -> torch.Tensor:
    """the update stage's P-hat (and the P stage's P_prev) [n, r]: mantissa arm: one nonzero per row,
    at column 0 of row 0, the last column of the last row"""
    if arm == "int":
        return _ints(gen, (n, r), -2, 2)
    if arm == "normal":
        return torch.randn((n, r), generator=gen)
    P = torch.zeros(n, r)
    col = torch.randint(0, r, (n,), generator=gen)
    col[0], col[n - 1] = 0, r - 1
    P[torch.arange(n), col] = _pow2(gen, (n,))
    return P


# constants of the element chain: powers of two, so that s * a is exact in the mantissa arm
MOMENTUM, LR = 0.5, 0.25
WD = 0.5


def int_bound(stage: str, n: int, m: int, r: int) -> float:
    """the largest magnitude an accumulator of the int arm can hold (inputs at their limits)"""
    worst_m = 3 + (3 + r * 2 * 2)  # g + (e - P_prev Qs^T)
    if stage == "p":
        return m * worst_m * 2
    if stage == "q":
        return n * worst_m * 2
    out = r * 2 * 2
    d = out + WD * 3
    mm = MOMENTUM * 3 + d
    return 3 + LR * (d + mm) + worst_m
