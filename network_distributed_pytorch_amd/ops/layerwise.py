"""LAMB and LARS on gfx950 (csrc/layerwise.hip): the layer-wise trust-ratio optimisers of large-batch
training over any number of fp32 tensors, in TWO launches per step (``lw_norm``: per-tensor fp64 norms
and the trust ratios, LAMB's moments and block; ``lw_apply``: the weights), both capture-safe.

The rules, for parameter tensors ``x_t``, gradients ``g_t``, ``div >= 1`` (by value), ``lr`` and ``wd``
from the hyper block (ops/hyper.py).  ``adapts_t`` is False for an exempt tensor (``adapt_mask``; the
gradient syncs exempt tensors of at most one dimension when ``decay_1d=False``): it gets neither decay
nor layer adaptation (trust 1), the usual exclusion of biases and norm weights.  Everything is fp32
and every line one correctly rounded operation unless marked; ``gg = g / div if div != 1 else g``.

LAMB (You et al. 2020, with bias correction), moments ``m``, ``v`` (zero at start), the 16-byte block
``{b1pow, b2pow, steps}`` and the scalars ``p1, p2, bc1, sb, om1, om2`` of :func:`ops.adamw.adamw_scalars`::

    m' = (beta1 m) + (om1 gg)          v' = (beta2 v) + (om2 (gg gg))      (bitwise the AdamW rule's)
    den = (sqrt(v') / sb) + eps        q = m' / den         r = q / bc1
    u = r + (wd x)  if wd != 0 and adapts_t else r
    W = sqrt(sum x^2), U = sqrt(sum u^2)                                     (fp64, per tensor)
    trust_t = float32(W / U)  if adapts_t and W > 0 and U > 0 else 1         (a NaN fails the tests)
    a = lr trust_t                     x' = x - (a u)

and once per step the block becomes ``{p1, p2, steps + 1}``.

LARS (You et al. 2017, the scaled-gradient form of LARC / lightning-bolts), ``eta = lars_coef``,
``eps_l = lars_eps``, momentum ``mu`` and buffer ``b`` (zero at start)::

    W = sqrt(sum x^2), G = sqrt(sum gg^2)                                    (fp64, per tensor)
    lam_t = float32((eta W) / ((G + (wd W)) + eps_l))  if adapts_t and W > 0 and G > 0 else 1
            (fp64 on the fp32 values of eta, wd, eps_l; rounded once)
    d = fma(wd, x, gg)  if wd != 0 and adapts_t else gg                      (the dense arm's decay rule)
    s = lam_t d           b' = fma(b, mu, s)           x' = fma(-lr, b', x)

The two fmas are the ones the dense arm's momentum-SGD kernel executes, so where ``lam_t == 1`` the
element rule is bitwise ``sgd_momentum_``'s.

The norm sums are fp64 (``acc = fma(v, v, acc)``) in a fixed order on the device (lane, wave butterfly,
the four waves in order, then a tensor's block partials in an order that depends on its size alone:
layerwise.hip's header), so a step is bitwise reproducible from run to run and under graph replay.

CPU tensors run the torch twin: the same operations in the same order except inside the fp64 sums
(torch's own summation order), and LARS's three fmas are emulated as an exact fp64 product, one fp64
add and one rounding to fp32, which differs from a true fma only by double rounding (about 2^-29 of
random inputs).  LAMB's twin has no fma: outside ``trust_t`` it is bitwise the device rule.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _UPLOADS, StateBlock, capturing, upload
from ._ext import ext
from .adamw import _sqrt, adamw_scalars, check_adam_args
from .hyper import HyperState

__all__ = ["FusedLamb", "FusedLars", "LayerwiseCore", "check_lars_args", "KINDS"]

F = np.float32
KINDS = ("lamb", "lars")


def check_lars_args(lars_coef, lars_eps) -> tuple:
    """``(lars_coef, lars_eps)`` as Python floats, or a ``ValueError``: both finite and > 0 as fp32."""
    try:
        coef, eps_l = float(lars_coef), float(lars_eps)
    except (TypeError, ValueError):
        raise ValueError(f"LARS: lars_coef and lars_eps must be numbers, got {lars_coef!r}, {lars_eps!r}") from None
    for name, val in (("lars_coef", coef), ("lars_eps", eps_l)):
        if not (F(val) > F(0.0)) or not math.isfinite(val) or not np.isfinite(F(val)):  # NaN fails the comparison
            raise ValueError(f"LARS: {name} must be a finite number > 0 as fp32, got {val}")
    return coef, eps_l


def _sumsq(t: torch.Tensor) -> float:
    d = t.double()
    return float(torch.dot(d, d))


def _fma(a: torch.Tensor, s: float, c: torch.Tensor) -> torch.Tensor:
    """``fma(a, s, c)`` on fp32 CPU tensors: exact fp64 product, one fp64 add, one rounding to fp32."""
    return torch.add(torch.mul(a.double(), float(F(s))), c.double()).float()


def _lamb_twin_(x, g, m, v, S, lr, wd, beta1, beta2, eps, div, adapts: bool) -> np.float32:
    """One tensor of the LAMB rule on flat CPU tensors, in place; returns ``trust_t``."""
    gg = torch.div(g, torch.tensor(div, dtype=torch.float32)) if F(div) != F(1.0) else g
    mn = torch.add(torch.mul(m, float(F(beta1))), torch.mul(gg, float(S["om1"])))
    vn = torch.add(torch.mul(v, float(F(beta2))), torch.mul(torch.mul(gg, gg), float(S["om2"])))
    den = torch.add(torch.div(_sqrt(vn), torch.tensor(float(S["sb"]), dtype=torch.float32)), float(F(eps)))
    u = torch.div(torch.div(mn, den), torch.tensor(float(S["bc1"]), dtype=torch.float32))
    if adapts and F(wd) != F(0.0):
        u = torch.add(u, torch.mul(x, float(F(wd))))
    with np.errstate(all="ignore"):
        W, U = np.sqrt(np.float64(_sumsq(x))), np.sqrt(np.float64(_sumsq(u)))
        trust = F(W / U) if adapts and W > 0 and U > 0 else F(1.0)
        a = F(lr) * trust
    x.copy_(torch.sub(x, torch.mul(u, float(a))))
    m.copy_(mn)
    v.copy_(vn)
    return trust


def _lars_twin_(x, g, b, lr, wd, mu, coef, eps_l, div, adapts: bool) -> np.float32:
    """One tensor of the LARS rule on flat CPU tensors, in place; returns ``lam_t``."""
    gg = torch.div(g, torch.tensor(div, dtype=torch.float32)) if F(div) != F(1.0) else g
    with np.errstate(all="ignore"):
        W, G = np.sqrt(np.float64(_sumsq(x))), np.sqrt(np.float64(_sumsq(gg)))
        lam = F(1.0)
        if adapts and W > 0 and G > 0:
            lam = F((np.float64(F(coef)) * W) / ((G + np.float64(F(wd)) * W) + np.float64(F(eps_l))))
    d = _fma(x, wd, gg) if adapts and F(wd) != F(0.0) else gg
    bn = _fma(b, mu, torch.mul(d, float(lam)))
    x.copy_(_fma(bn, -float(F(lr)), x))
    b.copy_(bn)
    return lam


class LayerwiseCore:
    """The two launches and their state over given arenas (flat fp32, never re-allocated): ``kind="lamb"``
    with the moment arenas ``m`` / ``v`` and ``beta1, beta2, eps``; ``kind="lars"`` with the momentum arena
    ``m`` (``v`` None) and ``mu, coef, eps_l``.  On a device the table (``capacity`` entries), the two-level
    arrival tickets and the fp64 partial pairs for up to ``max_blocks`` workgroups, the ``trust`` tensor
    (fp32, one per entry) and LAMB's 16-byte block are all allocated here, before any capture; on CPU the
    block is a dict and :meth:`run` is the torch twin.

    ``bind(rows)``: ``rows`` of ``(g, x, off, adapts)``, ONE per parameter tensor (the row index is the
    tensor index of ``trust``), g / x flat fp32 tensors of equal size, the tensor's moments at
    ``m[off: off + numel]``.  The device table is re-uploaded only when an address changed.
    """

    def __init__(self, device, kind: str, m: torch.Tensor, v: Optional[torch.Tensor], capacity: int, max_blocks: int,
                 **hp: float):
        if kind not in KINDS:
            raise ValueError(f"layer-wise optimiser: unknown kind {kind!r} ({', '.join(KINDS)})")
        self.device = torch.device(device)
        self.cuda = self.device.type == "cuda"
        self.kind, self.lamb = kind, kind == "lamb"
        assert m.dtype == torch.float32 and m.is_contiguous()
        assert (v is not None) == self.lamb
        if self.lamb:
            assert v.dtype == torch.float32 and v.is_contiguous() and v.numel() == m.numel()
            self.beta1, self.beta2, self.eps = check_adam_args((hp.pop("beta1"), hp.pop("beta2")), hp.pop("eps"))
        else:
            self.mu = float(hp.pop("mu"))
            self.coef, self.eps_l = check_lars_args(hp.pop("coef"), hp.pop("eps_l"))
        assert not hp, f"unused hyper-parameters {sorted(hp)}"
        self.m, self.v = m, v
        self.rows: List[tuple] = []
        self._key = None
        self._n_ent = self._n_blocks = 0
        self._cap = max(int(capacity), 1)
        self.state = StateBlock(self.device, ("b1pow", "b2pow", "steps"), (1.0, 1.0, 0)) if self.lamb else None
        self.block = self.state.dev if self.lamb else None
        self.trust = torch.ones(self._cap, dtype=torch.float32, device=self.device)
        if self.cuda:
            assert not capturing(), "the LAMB / LARS tables are built before capture"
            X = ext()
            self._max_blocks = max(int(max_blocks), 1)
            self._ent = torch.empty(self._cap * X.SIZEOF_SEGENTRY, dtype=torch.uint8, device=self.device)
            self._prefix = torch.empty(self._cap, dtype=torch.int64, device=self.device)
            self._partial = torch.zeros(2 * self._max_blocks, dtype=torch.float64, device=self.device)
            self.ctr = torch.zeros(X.arrive_ctr_words(self._max_blocks), dtype=torch.int32, device=self.device)

    def bind(self, rows: Sequence[tuple]) -> None:
        rows = list(rows)
        who = self.kind.upper()
        if len(rows) > self._cap:
            raise ValueError(f"{who}: {len(rows)} tensors exceed the capacity reserved at construction ({self._cap})")
        for g, x, off, _ in rows:
            if x.numel() == 0:
                raise ValueError(f"{who}: an empty tensor has no norm")
            if g.numel() != x.numel():
                raise ValueError(f"{who}: gradient of {g.numel()} elements for a parameter of {x.numel()}")
            if off < 0 or off + x.numel() > self.m.numel():
                raise ValueError(f"{who}: a tensor's moments lie outside the moment arenas")
            for t in (g, x):
                if t.device != self.device:
                    raise ValueError(f"{who} on {self.device}: tensor on {t.device}")
                if t.dtype != torch.float32 or not t.is_contiguous():
                    raise ValueError(f"{who}: tensors must be contiguous float32 "
                                     f"(got {t.dtype}, contiguous={t.is_contiguous()})")
        self.rows = rows
        if not self.cuda:
            return
        v_ptr = self.v.data_ptr() if self.lamb else self.m.data_ptr()
        key = (_UPLOADS.epoch, self.m.data_ptr(), v_ptr) + tuple(
            (g.data_ptr(), x.data_ptr(), x.numel(), int(off), bool(ad)) for g, x, off, ad in rows)
        if key == self._key:
            return
        ent, prefix, n_ent, n_blocks = ext().make_adamw_table(list(key[3:]), self.m.data_ptr(), v_ptr, self.m.numel())
        assert n_ent == len(rows)
        if n_blocks > self._max_blocks:
            raise ValueError(f"{who}: table of {n_blocks} blocks exceeds the capacity reserved at construction "
                             f"({self._max_blocks})")
        upload(self._ent, ent)
        upload(self._prefix, prefix)
        self._key, self._n_ent, self._n_blocks = key, int(n_ent), int(n_blocks)

    def run(self, lr: float, wd: float, div: float, hyper: Optional[torch.Tensor]) -> None:
        """One step over the bound rows: two launches on the current stream reading ``hyper`` (the
        device block; ``lr`` / ``wd`` are then ignored), or the twin on CPU."""
        if float(F(div)) < 1.0:
            raise ValueError(f"{self.kind.upper()}: div must be >= 1, got {div}")
        if self.cuda:
            if not self._n_blocks:
                raise RuntimeError(f"{self.kind.upper()}: empty table (bind() first)")
            assert hyper is not None, "the LAMB / LARS kernels always read lr / weight_decay from a device block"
            hp = (dict(beta1=self.beta1, beta2=self.beta2, eps=self.eps, mu=0.0, coef=0.0, eps_l=0.0) if self.lamb else
                  dict(beta1=0.0, beta2=0.0, eps=0.0, mu=self.mu, coef=self.coef, eps_l=self.eps_l))
            tab = (self._ent, self._prefix, self._n_ent, self._n_blocks)
            tail = dict(hyper=hyper, m=self.m, v=self.v, block=self.block, div=float(div), **hp)
            ext().lw_norm(self.lamb, *tab, self._partial, self.ctr, self.trust, **tail)
            ext().lw_apply(self.lamb, *tab, self.trust, **tail)
            return
        with torch.no_grad():
            if self.lamb:
                st = self.state.read()
                S = adamw_scalars(st["b1pow"], st["b2pow"], lr, wd, self.beta1, self.beta2)
                for t, (g, x, off, ad) in enumerate(self.rows):
                    n = x.numel()
                    self.trust[t] = float(_lamb_twin_(x.view(-1), g.reshape(-1), self.m[off: off + n],
                                                      self.v[off: off + n], S, lr, wd, self.beta1, self.beta2,
                                                      self.eps, float(div), bool(ad)))
                self.state.write({"b1pow": float(S["p1"]), "b2pow": float(S["p2"]), "steps": st["steps"] + 1})
            else:
                for t, (g, x, off, ad) in enumerate(self.rows):
                    self.trust[t] = float(_lars_twin_(x.view(-1), g.reshape(-1), self.m[off: off + x.numel()], lr, wd,
                                                      self.mu, self.coef, self.eps_l, float(div), bool(ad)))

    # ---- state ----------------------------------------------------------------------------------
    def trust_ratios(self) -> torch.Tensor:
        """``trust_t`` / ``lam_t`` of the last step, one per bound tensor, on the CPU: a host sync."""
        return self.trust[: len(self.rows)].detach().cpu().clone()

    def read(self) -> Optional[Dict[str, Any]]:
        """LAMB: ``{"b1pow", "b2pow", "steps"}`` (a host sync on a device); LARS keeps no block: None."""
        return self.state.read() if self.lamb else None

    def write(self, st: Dict[str, Any]) -> None:
        if self.lamb:
            self.state.write({"b1pow": float(F(st["b1pow"])), "b2pow": float(F(st["b2pow"])), "steps": st["steps"]})

    def snapshot(self):
        return self.trust.clone(), (self.state.snapshot() if self.lamb else None)

    def restore(self, snap) -> None:
        self.trust.copy_(snap[0])
        if self.lamb:
            self.state.restore(snap[1])


class _FusedLayerwise(HyperState):
    """What :class:`FusedLamb` and :class:`FusedLars` share: the flat fp32 state arenas, in which every
    tensor's state sits as far past a 16-byte boundary as its parameter (an aligned parameter keeps the
    float4 path), one table entry per parameter, the :class:`LayerwiseCore` and a :class:`HyperBlock`
    (the :class:`HyperState` protocol; the kernels always read it).  Everything exists after
    construction, which is eager; :meth:`step` is two launches and capture-safe; CPU runs the twin."""

    _kind = ""

    def __init__(self, params: Sequence[torch.Tensor], lr: float, weight_decay: float,
                 adapt_mask: Optional[Sequence[bool]], **hp: float):
        self._arm = type(self).__name__
        self.params: List[torch.Tensor] = [p.detach() for p in params]
        if not self.params:
            raise ValueError(f"{self._arm}: no parameters")
        lr, wd = float(lr), float(weight_decay)
        if not (math.isfinite(lr) and lr >= 0.0) or not (math.isfinite(wd) and wd >= 0.0):
            raise ValueError(f"{self._arm}: lr and weight_decay must be finite and >= 0, got {lr}, {wd}")
        self.adapts = [True] * len(self.params) if adapt_mask is None else [bool(d) for d in adapt_mask]
        if len(self.adapts) != len(self.params):
            raise ValueError(f"{self._arm}: adapt_mask of {len(self.adapts)} for {len(self.params)} parameters")
        self.device = self.params[0].device
        cuda = self.device.type == "cuda"
        if cuda:
            assert not capturing(), f"{self._arm} is built before capture"
        self.offsets: List[int] = []
        total = 0
        for p in self.params:
            if p.device != self.device:
                raise ValueError(f"{self._arm} on {self.device}: tensor on {p.device}")
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError(f"{self._arm}: tensors must be contiguous float32 "
                                 f"(got {p.dtype}, contiguous={p.is_contiguous()})")
            total = (total + 3) // 4 * 4 + (p.data_ptr() % 16) // 4
            self.offsets.append(total)
            total += p.numel()
        f32 = dict(dtype=torch.float32, device=self.device)
        lamb = self._kind == "lamb"
        self.m_arena = torch.zeros(max(total, 1), **f32)
        self.v_arena = torch.zeros(max(total, 1), **f32) if lamb else None
        blocks = sum((p.numel() + 2047) // 2048 for p in self.params)
        self.core = LayerwiseCore(self.device, self._kind, self.m_arena, self.v_arena, len(self.params), blocks, **hp)
        self._init_hyper(float(F(lr)), float(F(wd)), block=cuda, on=True)
        self._bound = False

    def _views(self, arena: torch.Tensor) -> List[torch.Tensor]:
        return [arena[o: o + p.numel()].view(p.shape) for o, p in zip(self.offsets, self.params)]

    def bind(self, grads: Sequence[torch.Tensor]) -> None:
        """The gradients of the coming steps, one per parameter, in order."""
        grads = list(grads)
        if len(grads) != len(self.params):
            raise ValueError(f"{self._arm}.bind: {len(grads)} gradients for {len(self.params)} parameters")
        if any(g is None for g in grads):
            raise ValueError(f"{self._arm}.bind: a gradient is None")
        self.core.bind([(g.reshape(-1) if g.is_contiguous() else g, p.view(-1), off, ad)
                        for g, p, off, ad in zip(grads, self.params, self.offsets, self.adapts)])
        self._bound = True

    def step(self, div: float = 1.0) -> None:
        """One step over the bound gradients: two launches on a device (current stream), the twin on CPU."""
        if not self._bound:
            raise RuntimeError(f"{self._arm}.step: bind() the gradients first")
        self.core.run(self.lr, self.weight_decay, div, self._hyper_arg())

    def trust_ratios(self) -> torch.Tensor:
        """The last step's per-tensor ratios, one per parameter, on the CPU: a host sync."""
        return self.core.trust_ratios()

    def read(self) -> Optional[Dict[str, Any]]:
        return self.core.read()

    def snapshot(self):
        """State arenas, trust ratios and block, for :meth:`restore` (a graph warm-up leaves no trace)."""
        return self.m_arena.clone(), (self.v_arena.clone() if self.v_arena is not None else None), self.core.snapshot()

    def restore(self, snap) -> None:
        m, v, core = snap
        self.m_arena.copy_(m)
        if self.v_arena is not None:
            self.v_arena.copy_(v)
        self.core.restore(core)

    def _load_lists(self, sd: Dict[str, Any], pairs) -> None:
        for key, mine in pairs:
            vals = list(sd[key])
            if len(vals) != len(mine) or any(tuple(a.shape) != tuple(b.shape) for a, b in zip(vals, mine)):
                raise ValueError(f"{self._arm}.load_state_dict: {key} does not match the parameters")
        with torch.no_grad():
            for key, mine in pairs:
                for t, val in zip(mine, sd[key]):
                    t.copy_(val)
        self._load_hyper(float(F(sd["lr"])), float(F(sd.get("weight_decay", self.weight_decay))))


class FusedLamb(_FusedLayerwise):
    """The LAMB of the module docstring over ``params`` (tensors updated in place; never re-targeted),
    ``adapt_mask[i]`` False exempting tensor ``i`` from the decay and the layer adaptation.
    ``exp_avg`` / ``exp_avg_sq`` are views shaped like ``params``."""

    _kind = "lamb"

    def __init__(self, params, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 adapt_mask: Optional[Sequence[bool]] = None):
        b1, b2, eps = check_adam_args(betas, eps)
        super().__init__(params, lr, weight_decay, adapt_mask, beta1=b1, beta2=b2, eps=eps)
        self.exp_avg, self.exp_avg_sq = self._views(self.m_arena), self._views(self.v_arena)

    def state_dict(self) -> Dict[str, Any]:
        st = self.read()
        return {"optimizer": "lamb", "exp_avg": [t.detach().cpu().clone() for t in self.exp_avg],
                "exp_avg_sq": [t.detach().cpu().clone() for t in self.exp_avg_sq], **st,
                "lr": self.lr, "weight_decay": self.weight_decay, "betas": (self.core.beta1, self.core.beta2),
                "eps": self.core.eps}

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        self._load_lists(sd, (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)))
        self.core.write(sd)


class FusedLars(_FusedLayerwise):
    """The LARS of the module docstring over ``params``; ``momentum_buffer`` are views shaped like them."""

    _kind = "lars"

    def __init__(self, params, lr: float, momentum: float = 0.9, weight_decay: float = 0.0, lars_coef: float = 0.001,
                 lars_eps: float = 1e-8, adapt_mask: Optional[Sequence[bool]] = None):
        if not 0.0 <= float(momentum) < 1.0:
            raise ValueError(f"FusedLars: momentum must be in [0, 1), got {momentum}")
        coef, eps_l = check_lars_args(lars_coef, lars_eps)
        super().__init__(params, lr, weight_decay, adapt_mask, mu=float(momentum), coef=coef, eps_l=eps_l)
        self.momentum_buffer = self._views(self.m_arena)

    def state_dict(self) -> Dict[str, Any]:
        return {"optimizer": "lars", "momentum_buffer": [t.detach().cpu().clone() for t in self.momentum_buffer],
                "lr": self.lr, "weight_decay": self.weight_decay, "momentum": self.core.mu,
                "lars_coef": self.core.coef, "lars_eps": self.core.eps_l}

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        self._load_lists(sd, (("momentum_buffer", self.momentum_buffer),))
