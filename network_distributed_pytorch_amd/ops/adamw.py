"""AdamW on gfx950 (csrc/adamw.hip): ``torch.optim.AdamW`` (decoupled weight decay, bias
correction) over any number of fp32 tensors in ONE launch whose step-dependent bias corrections
live on the device, so a captured step serves every step.

The rule (bitwise identical on the device and in the torch twin that CPU tensors run), for
parameters ``x_i``, gradients ``g_i``, moments ``m_i``, ``v_i`` (zero at start), ``beta1``,
``beta2`` in [0, 1), ``eps > 0`` and ``div >= 1`` (by value: frozen into a captured graph),
``lr`` and ``wd`` from the hyper block (ops/hyper.py) and the 16-byte block
``{float b1pow; float b2pow; uint32 steps; uint32 pad}``, which starts as ``{1, 1, 0, 0}``.
Every line is one correctly rounded fp32 operation; nothing is fused.

Per launch, from the block as it was before the launch (:func:`adamw_scalars`)::

    p1 = b1pow * beta1      p2 = b2pow * beta2
    bc1 = 1 - p1            bc2 = 1 - p2
    ss = lr / bc1           sb = sqrt(bc2)
    om1 = 1 - beta1         om2 = 1 - beta2
    c = 1 - lr * wd

Per element::

    gg = g / div  if div != 1 else g
    x1 = x * c    if wd != 0 and the tensor decays else x
    m' = (beta1 * m) + (om1 * gg)
    v' = (beta2 * v) + (om2 * (gg * gg))
    den = (sqrt(v') / sb) + eps
    x' = x1 - ss * (m' / den)

Once per launch the block becomes ``{p1, p2, steps + 1, 0}``.  The running products replace
``pow(beta, t)``: one fp32 multiply per step is bitwise reproducible between the device and the
twin, ``powf`` is not, and the step count never visits the host.  ``g = m = v = 0`` leaves ``x1``
unchanged; NaN and inf propagate.  ``amsgrad``, ``maximize`` and coupled-L2 Adam are not offered.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _UPLOADS, StateBlock, capturing, upload
from ._ext import ext
from .hyper import HyperState

__all__ = ["FusedAdamW", "AdamWCore", "adamw_scalars", "check_adam_args"]

F = np.float32


def check_adam_args(betas, eps) -> tuple:
    """``(beta1, beta2, eps)`` as Python floats, or a ``ValueError``: betas in [0, 1) and
    ``eps > 0``, both as fp32 (what the kernel receives)."""
    try:
        b1, b2 = (float(b) for b in betas)
        eps = float(eps)
    except (TypeError, ValueError):
        raise ValueError(f"AdamW: betas must be two numbers and eps a number, got {betas!r}, {eps!r}") from None
    for name, b in (("beta1", b1), ("beta2", b2)):
        if not (F(0.0) <= F(b) < F(1.0)):  # NaN fails both comparisons
            raise ValueError(f"AdamW: {name} must be in [0, 1) as fp32, got {b}")
    if not (F(eps) > F(0.0)) or math.isinf(eps):
        raise ValueError(f"AdamW: eps must be a finite number > 0 as fp32, got {eps}")
    return b1, b2, eps


def adamw_scalars(b1pow, b2pow, lr, wd, beta1, beta2) -> Dict[str, np.float32]:
    """The per-launch scalars of the rule as ``numpy.float32``, from the block before the launch:
    the Python twin of the kernel's schedule."""
    with np.errstate(all="ignore"):
        p1 = F(b1pow) * F(beta1)
        p2 = F(b2pow) * F(beta2)
        bc1 = F(1.0) - p1
        bc2 = F(1.0) - p2
        ss = F(lr) / bc1
        sb = np.sqrt(bc2)
        om1 = F(1.0) - F(beta1)
        om2 = F(1.0) - F(beta2)
        lw = F(lr) * F(wd)
        c = F(1.0) - lw
    out = dict(p1=p1, p2=p2, bc1=bc1, bc2=bc2, ss=ss, sb=sb, om1=om1, om2=om2, c=c)
    assert all(v.dtype == F for v in out.values())
    return out


def _sqrt(t: torch.Tensor) -> torch.Tensor:
    """The correctly rounded fp32 square root of a CPU tensor.  ``torch.sqrt`` is not it: its
    vectorised CPU kernel is off by one ulp on about 0.7 % of normal-range inputs (measured against
    the fp64 root rounded once, which numpy's hardware ``sqrt`` equals on every input tried)."""
    with np.errstate(all="ignore"):
        return torch.from_numpy(np.sqrt(t.contiguous().numpy()))


def _twin_(x, g, m, v, S, beta1, beta2, eps, div, decays: bool) -> None:
    """The per-element rule on CPU tensors with mul / add / sub / div / sqrt only (each rounds its
    fp32 result once; a Python scalar operand is taken as fp32)."""
    gg = torch.div(g, torch.tensor(div, dtype=torch.float32)) if F(div) != F(1.0) else g
    x1 = torch.mul(x, float(S["c"])) if decays else x
    a = torch.mul(m, float(F(beta1)))
    b = torch.mul(gg, float(S["om1"]))
    mn = torch.add(a, b)
    g2 = torch.mul(gg, gg)
    d = torch.mul(v, float(F(beta2)))
    e = torch.mul(g2, float(S["om2"]))
    vn = torch.add(d, e)
    den = torch.add(torch.div(_sqrt(vn), torch.tensor(float(S["sb"]), dtype=torch.float32)), float(F(eps)))
    u = torch.mul(torch.div(mn, den), float(S["ss"]))
    x.copy_(torch.sub(x1, u))
    m.copy_(mn)
    v.copy_(vn)


class AdamWCore:
    """The launch and its state over two given moment arenas ``m`` / ``v`` (flat fp32, equal size,
    never re-allocated): on a device the table (``capacity`` entries), the two-level arrival
    tickets for up to ``max_blocks`` workgroups and the 16-byte block, all allocated here, before
    any capture; on CPU the block as a dict and the torch twin.  :class:`FusedAdamW` and the
    dense gradient sync (parallel/ddp.py) are built on it.

    ``bind(rows)``: ``rows`` of ``(g, x, off, decays)``, g / x flat fp32 tensors of equal size,
    the entry's moments at ``m[off: off + numel]`` / ``v[...]``.  The device table is re-uploaded
    only when an address changed (capture-safe through :func:`ops.upload`).
    """

    def __init__(self, device, m: torch.Tensor, v: torch.Tensor, capacity: int, max_blocks: int):
        self.device = torch.device(device)
        self.cuda = self.device.type == "cuda"
        assert m.dtype == torch.float32 and v.dtype == torch.float32 and m.numel() == v.numel()
        assert m.is_contiguous() and v.is_contiguous()
        self.m, self.v = m, v
        self.rows: List[tuple] = []
        self._key = None
        self._n_ent = self._n_blocks = 0
        self.state = StateBlock(self.device, ("b1pow", "b2pow", "steps"), (1.0, 1.0, 0))
        self.block = self.state.dev  # the kernel's argument (None on CPU: the twin keeps a dict)
        if self.cuda:
            assert not capturing(), "the AdamW tables are built before capture"
            X = ext()
            self._cap = max(int(capacity), 1)
            self._max_blocks = max(int(max_blocks), 1)
            self._ent = torch.empty(self._cap * X.SIZEOF_SEGENTRY, dtype=torch.uint8, device=self.device)
            self._prefix = torch.empty(self._cap, dtype=torch.int64, device=self.device)
            self.ctr = torch.zeros(X.arrive_ctr_words(self._max_blocks), dtype=torch.int32, device=self.device)

    def bind(self, rows: Sequence[tuple]) -> None:
        rows = list(rows)
        for g, x, off, _ in rows:
            if g.numel() != x.numel():
                raise ValueError(f"AdamW: gradient of {g.numel()} elements for a parameter of {x.numel()}")
            if off < 0 or off + x.numel() > self.m.numel():
                raise ValueError("AdamW: an entry's moments lie outside the moment arenas")
            for t in (g, x):
                if t.device != self.device:
                    raise ValueError(f"AdamW on {self.device}: tensor on {t.device}")
                if t.dtype != torch.float32 or not t.is_contiguous():
                    raise ValueError("AdamW: tensors must be contiguous float32 "
                                     f"(got {t.dtype}, contiguous={t.is_contiguous()})")
        self.rows = rows
        if not self.cuda:
            return
        key = (_UPLOADS.epoch, self.m.data_ptr(), self.v.data_ptr()) + tuple(
            (g.data_ptr(), x.data_ptr(), x.numel(), int(off), bool(dec)) for g, x, off, dec in rows)
        if key == self._key:
            return
        ent, prefix, n_ent, n_blocks = ext().make_adamw_table(list(key[3:]), self.m.data_ptr(), self.v.data_ptr(),
                                                              self.m.numel())
        if n_ent > self._cap or n_blocks > self._max_blocks:
            raise ValueError(f"AdamW: table of {n_ent} entries / {n_blocks} blocks exceeds the capacity "
                             f"reserved at construction ({self._cap} / {self._max_blocks})")
        upload(self._ent, ent)
        upload(self._prefix, prefix)
        self._key, self._n_ent, self._n_blocks = key, int(n_ent), int(n_blocks)

    def run(self, lr: float, wd: float, beta1: float, beta2: float, eps: float, div: float,
            hyper: Optional[torch.Tensor]) -> None:
        """One run of the rule over the bound rows: one launch on the current stream reading
        ``hyper`` (the device block; ``lr`` / ``wd`` are then ignored), or the twin on CPU."""
        if float(F(div)) < 1.0:
            raise ValueError(f"AdamW: div must be >= 1, got {div}")
        if self.cuda:
            if not self._n_blocks:
                raise RuntimeError("AdamW: empty table (bind() first)")
            assert hyper is not None, "the AdamW kernel always reads lr / weight_decay from a device block"
            ext().adamw_step(self._ent, self._prefix, self._n_ent, self._n_blocks, self.ctr, self.block, hyper,
                             self.m, self.v, float(beta1), float(beta2), float(eps), float(div))
            return
        st = self.state.read()
        S = adamw_scalars(st["b1pow"], st["b2pow"], lr, wd, beta1, beta2)
        with torch.no_grad():
            for g, x, off, dec in self.rows:
                n = x.numel()
                _twin_(x.view(-1), g.reshape(-1), self.m[off: off + n], self.v[off: off + n], S, beta1, beta2, eps,
                       float(div), bool(dec) and F(wd) != F(0.0))
        self.state.write({"b1pow": float(S["p1"]), "b2pow": float(S["p2"]), "steps": st["steps"] + 1})

    # ---- the block ----------------------------------------------------------------------------
    def read(self) -> Dict[str, Any]:
        """``{"b1pow", "b2pow", "steps"}``: a host sync on a device."""
        return self.state.read()

    def write(self, st: Dict[str, Any]) -> None:
        self.state.write({"b1pow": float(F(st["b1pow"])), "b2pow": float(F(st["b2pow"])), "steps": st["steps"]})

    def snapshot(self):
        return self.state.snapshot()

    def restore(self, snap) -> None:
        self.state.restore(snap)


class FusedAdamW(HyperState):
    """The AdamW of the module docstring over ``params`` (tensors updated in place; never
    re-targeted), ``decay_mask[i]`` False exempting tensor ``i`` from the weight decay.

    Owns the two flat fp32 moment arenas, in which every moment sits as far past a 16-byte
    boundary as its parameter (an aligned parameter keeps the float4 path), ``exp_avg`` /
    ``exp_avg_sq`` (views shaped like ``params``), and on a device the table, the tickets, the
    state block and a :class:`HyperBlock` (the :class:`HyperState` protocol; the kernel always reads it).  Everything exists after construction, which is eager;
    :meth:`step` is one launch and capture-safe.  On a CPU device the same class runs the twin.
    """

    _arm = "FusedAdamW"

    def __init__(self, params: Sequence[torch.Tensor], lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, decay_mask: Optional[Sequence[bool]] = None):
        self.params: List[torch.Tensor] = [p.detach() for p in params]
        if not self.params:
            raise ValueError("FusedAdamW: no parameters")
        self.beta1, self.beta2, self.eps = check_adam_args(betas, eps)
        lr, wd = float(lr), float(weight_decay)
        if not (math.isfinite(lr) and lr >= 0.0) or not (math.isfinite(wd) and wd >= 0.0):
            raise ValueError(f"FusedAdamW: lr and weight_decay must be finite and >= 0, got {lr}, {wd}")
        self.decays = [True] * len(self.params) if decay_mask is None else [bool(d) for d in decay_mask]
        if len(self.decays) != len(self.params):
            raise ValueError(f"FusedAdamW: decay_mask of {len(self.decays)} for {len(self.params)} parameters")
        self.device = self.params[0].device
        cuda = self.device.type == "cuda"
        if cuda:
            assert not capturing(), "FusedAdamW is built before capture"
        for p in self.params:
            if p.device != self.device:
                raise ValueError(f"FusedAdamW on {self.device}: tensor on {p.device}")
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError("FusedAdamW: tensors must be contiguous float32 "
                                 f"(got {p.dtype}, contiguous={p.is_contiguous()})")
        # moment offsets (floats): a parameter that follows its predecessor in memory follows it
        # in the arenas too; otherwise it starts as far past a 16-byte boundary as its own memory
        self.offsets: List[int] = []
        total, prev_end = 0, None
        for p in self.params:
            if prev_end is None or p.data_ptr() != prev_end or p.numel() == 0:
                total = (total + 3) // 4 * 4 + (p.data_ptr() % 16) // 4
            self.offsets.append(total)
            total += p.numel()
            prev_end = p.data_ptr() + 4 * p.numel() if p.numel() else None
        f32 = dict(dtype=torch.float32, device=self.device)
        self.m_arena = torch.zeros(max(total, 1), **f32)
        self.v_arena = torch.zeros(max(total, 1), **f32)
        assert self.m_arena.data_ptr() % 16 == 0 and self.v_arena.data_ptr() % 16 == 0
        self.exp_avg = [self.m_arena[o: o + p.numel()].view(p.shape) for o, p in zip(self.offsets, self.params)]
        self.exp_avg_sq = [self.v_arena[o: o + p.numel()].view(p.shape) for o, p in zip(self.offsets, self.params)]
        blocks = sum((p.numel() + 2047) // 2048 for p in self.params)
        self.core = AdamWCore(self.device, self.m_arena, self.v_arena, len(self.params), blocks)
        self._init_hyper(float(F(lr)), float(F(wd)), block=cuda, on=True)
        self._bound = False

    # ---- the rule -----------------------------------------------------------------------------
    def bind(self, grads: Sequence[torch.Tensor]) -> None:
        """The gradients of the coming steps, one per parameter, in order.  Neighbours whose
        gradient, parameter and moments are all adjacent in memory and that decay alike share
        one table entry."""
        grads = list(grads)
        if len(grads) != len(self.params):
            raise ValueError(f"FusedAdamW.bind: {len(grads)} gradients for {len(self.params)} parameters")
        rows: List[list] = []
        for g, p, off, dec in zip(grads, self.params, self.offsets, self.decays):
            if g is None:
                raise ValueError("FusedAdamW.bind: a gradient is None")
            if g.dtype != torch.float32 or not g.is_contiguous() or g.device != self.device:
                raise ValueError("FusedAdamW.bind: gradients must be contiguous float32 on the parameters' device "
                                 f"(got {g.dtype}, contiguous={g.is_contiguous()}, {g.device})")
            if g.numel() != p.numel():
                raise ValueError(f"FusedAdamW.bind: gradient of {g.numel()} elements for a parameter of {p.numel()}")
            if p.numel() == 0:
                continue
            if rows:
                g0, p0, n0, off0, dec0 = rows[-1]
                if (dec0 == dec and off0 + n0 == off and p0.data_ptr() + 4 * n0 == p.data_ptr()
                        and g0.data_ptr() + 4 * n0 == g.data_ptr()
                        and p0.untyped_storage().data_ptr() == p.untyped_storage().data_ptr()
                        and g0.untyped_storage().data_ptr() == g.untyped_storage().data_ptr()):
                    rows[-1][2] += p.numel()
                    continue
            rows.append([g, p, p.numel(), off, dec])
        flat = []
        for g, p, n, off, dec in rows:
            gf = g.reshape(-1) if n == g.numel() else torch.as_strided(g, (n,), (1,))
            pf = p.view(-1) if n == p.numel() else torch.as_strided(p, (n,), (1,))
            flat.append((gf, pf, off, dec))
        self.core.bind(flat)
        self._bound = True

    def step(self, div: float = 1.0) -> None:
        """One run of the rule over the bound gradients: one launch on a device (current stream),
        the twin on CPU."""
        if not self._bound:
            raise RuntimeError("FusedAdamW.step: bind() the gradients first")
        self.core.run(self.lr, self.weight_decay, self.beta1, self.beta2, self.eps, div, self._hyper_arg())

    # ---- state --------------------------------------------------------------------------------
    def read(self) -> Dict[str, Any]:
        """``{"b1pow", "b2pow", "steps"}`` of the block: a host sync on a device."""
        return self.core.read()

    def snapshot(self):
        """Moments and block, for :meth:`restore` (a graph warm-up leaves no trace)."""
        return self.m_arena.clone(), self.v_arena.clone(), self.core.snapshot()

    def restore(self, snap) -> None:
        m, v, blk = snap
        self.m_arena.copy_(m)
        self.v_arena.copy_(v)
        self.core.restore(blk)

    def state_dict(self) -> Dict[str, Any]:
        """CPU tensors plus the block: ``{"exp_avg": [...], "exp_avg_sq": [...], "b1pow", "b2pow",
        "steps", "lr", "weight_decay", "betas", "eps"}``."""
        st = self.read()
        return {"exp_avg": [t.detach().cpu().clone() for t in self.exp_avg],
                "exp_avg_sq": [t.detach().cpu().clone() for t in self.exp_avg_sq],
                "b1pow": st["b1pow"], "b2pow": st["b2pow"], "steps": st["steps"],
                "lr": self.lr, "weight_decay": self.weight_decay, "betas": (self.beta1, self.beta2),
                "eps": self.eps}

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        for key, mine in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
            vals = list(sd[key])
            if len(vals) != len(mine):
                raise ValueError(f"FusedAdamW.load_state_dict: {len(vals)} {key} tensors for {len(mine)}")
            for t, val in zip(mine, vals):
                if tuple(val.shape) != tuple(t.shape):
                    raise ValueError(f"FusedAdamW.load_state_dict: shape {tuple(val.shape)} for {tuple(t.shape)}")
        with torch.no_grad():
            for key, mine in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
                for t, val in zip(mine, sd[key]):
                    t.copy_(val)
        self.core.write(sd)
        if "lr" in sd:
            self._load_hyper(float(F(sd["lr"])), float(F(sd.get("weight_decay", self.weight_decay))))
