"""``GradSync``: what every gradient-synchronisation strategy offers its callers (the engine,
``utils.graph.StepRunner``, ``utils.checkpoint``, ``bench.py``), written down once.

``build_grad_sync(kind, model, comm, ...)`` (parallel/trainer.py) returns one of:

=================  ===========================================================================
``powersgd``       fused native engine (:class:`PowerSGDOptimizer`): EF + PowerSGD + momentum
                   + SGD over flat arenas; on a device the per-group pipelines (6 gfx950
                   launches + 2 collectives each) overlap backward on the side stream.
``powersgd-adamw`` the same engine with AdamW in its update pass in the place of momentum SGD
                   (``optimizer="adamw"`` of :class:`PowerSGDOptimizer`; rank <= 16, full layout).
``powersgd-ref``   reference semantics, eager per-tensor loops (ddp_init.py:149-178 with the
                   reducer's torch path) — the "eager reference" comparison arm.
``dense``          bucketed all-reduce overlapped with backward + fused SGD-momentum kernel.
``dense-ref``      reference dense arm: blocking per-parameter all-reduce + torch.optim.SGD
                   (ddp_guide_cifar10/ddp_init.py:57-62,111,124-125).
=================  ===========================================================================

Every strategy has ``set_hyper(lr, weight_decay)``: the learning rate and the L2 weight decay of
the steps from now on (the engine calls it before every step when a schedule or a decay is on).
The native engines keep both in their optimiser's device block (ops/hyper.py ``HyperState``), the
reference loops apply it in torch.

Every strategy takes ``max_grad_norm`` (0: off; ``inf``: measure only) and has ``clip_stats()``: the
``{"norm", "coef", "clipped", "steps"}`` block of the global-norm gradient clip (ops/gradclip.py), or
None when clipping is off.  The PowerSGD arms clip each rank's own gradient before the error
feedback; the dense arms and the local optimisers clip the averaged gradient before the update.

Every strategy has ``attach_ema(ema)``: an ``ops.WeightEma`` (ops/ema.py) whose ``update()`` then
runs once per step, behind the step's last update launch and on its stream (inside a captured
step); the native engines' ``snapshot()`` / ``restore()`` include it.  Nothing attached: every
launch, snapshot and state dict is what it is without.

``optimizer="adamw"`` (with ``betas``, ``eps``, ``decay_1d``) replaces momentum SGD by AdamW
(ops/adamw.py) behind ``dense`` (the fused launch over the arenas), ``powersgd-ref`` / ``powersgd-api``
(``FusedAdamW`` over the decompressed, averaged gradients; error memory and wire untouched) and
``dense-ref`` (``torch.optim.AdamW`` with two param groups, capturable on a device); ``adam_stats()``
returns the step count.  ``powersgd`` and the local optimisers raise: the fused engine's Adam variant is
its own kind, ``powersgd-adamw`` (the kind is the optimiser choice, as ``local-adamw``).  With ``optimizer="sgd"``
every constructor call is exactly what it is without these arguments.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import torch

from ..ops import capturing
from ..ops.gradclip import GradClip

__all__ = ["GradSync"]


class GradSync:
    """Base of every strategy.  A subclass writes ``zero_grad()``, ``step() -> bits`` and
    ``set_hyper(lr, weight_decay=None)``, sets ``bytes_per_step`` / ``collectives_per_step`` and calls
    :meth:`_init_clip`; every other method here is the right answer for an arm that has nothing to
    say, and the clip / EMA plumbing is shared."""

    bytes_per_step = 0
    collectives_per_step = 0
    flat_weights: Optional[torch.Tensor] = None  # the flat parameter arena of the two native arms
    max_grad_norm = 0.0
    clip: Optional[GradClip] = None
    ema = None  # ops.WeightEma updated behind the step's last update launch (attach_ema)

    def zero_grad(self):
        raise NotImplementedError

    def step(self) -> int:
        raise NotImplementedError

    def set_hyper(self, lr: float, weight_decay: Optional[float] = None):
        raise NotImplementedError

    # -- defaults: an arm with nothing to say ------------------------------------------------------
    def plan_hyper(self, pairs) -> None:
        """The coming steps' ``(lr, weight_decay)`` pairs, for an arm that writes upload rows ahead."""

    def prepare(self) -> None:
        """Host-side work a graph warm-up snapshot must come after."""

    def count_step(self) -> None:
        """Host bookkeeping of one step; a graph replay, which skips the Python of ``step()``, calls it."""

    def check_errors(self) -> None:
        """Host-synchronising health check (low cadence); raises on a device-side or RCCL error."""

    def phases(self):
        """``[(fn, is_collective)]`` for piecewise capture and per-phase timing (calling it switches
        overlap off), or None: the step is one piece."""
        return None

    def collective_payloads(self) -> List[int]:
        """Bytes of every collective of one step, in issue order (link-model input)."""
        return []

    def adam_stats(self) -> Optional[Dict[str, Any]]:
        """The AdamW block (at least ``"steps"``; a host sync), or None with SGD."""
        return None

    def snapshot(self):
        """Training state for :meth:`restore` (a graph warm-up leaves no trace), or None."""
        return None

    def restore(self, snap) -> None:
        assert snap is None, "restore() of a snapshot this strategy never took"

    def state_dict(self):
        """Checkpoint state, or None for an arm that keeps none."""
        return None

    def load_state_dict(self, sd) -> None:
        pass

    # -- gradient clip and weight EMA, shared --------------------------------------------------------
    def _init_clip(self, max_grad_norm: float, device, **sizes) -> None:
        """``max_grad_norm`` and the :class:`GradClip` (``sizes``: its ``capacity`` / ``blocks``), built
        before any capture; None when clipping is off."""
        assert max_grad_norm >= 0, "max_grad_norm >= 0 (0: off, inf: measure only)"
        self.max_grad_norm = float(max_grad_norm)
        self.clip = GradClip(device, **sizes) if self.max_grad_norm > 0 else None

    def _clip_grads(self, grads, div: float = 1.0) -> None:
        """Clip ``grads`` in place by their global norm (device kernels or the torch twin)."""
        if self.clip is not None:
            self.clip.bind([g for g in grads if g is not None])
            self.clip.run(self.max_grad_norm, div)

    def clip_stats(self) -> Optional[Dict[str, Any]]:
        """``{"norm", "coef", "clipped", "steps"}`` of the gradient clip (a host sync), or None when
        ``max_grad_norm`` is 0.  The PowerSGD arms report this rank's own norm, the others that of
        the averaged gradient, equal on every rank."""
        return self.clip.read() if self.clip is not None else None

    def attach_ema(self, ema) -> None:
        """Keep ``ema`` (ops/ema.py) of the weights: one launch per step behind the step's last update
        launch, on its stream, inside a captured step; part of :meth:`snapshot` where there is one.
        None detaches."""
        assert not capturing(), "attach_ema() inside a graph capture"
        self.ema = ema

    def _after_update(self) -> None:
        """The tail of every step's last update launch, on its stream."""
        if self.ema is not None:
            self.ema.update()

    def _snapshot_extras(self) -> Dict[str, Any]:
        """The clip / EMA entries of a :meth:`snapshot`."""
        return {**({"clip": self.clip.snapshot()} if self.clip is not None else {}),
                **({"ema": self.ema.snapshot()} if self.ema is not None else {})}

    def _restore_extras(self, snap) -> None:
        if self.clip is not None:
            self.clip.restore(snap["clip"])
        if self.ema is not None and "ema" in snap:  # a snapshot from before attach_ema()
            self.ema.restore(snap["ema"])
