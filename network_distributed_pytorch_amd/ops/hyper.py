"""The optimisers' device-resident hyper-parameter block ``[lr, weight_decay, 0, 0]`` (csrc/hyper.h).

A captured training step freezes the by-value arguments of its update kernels into the hipGraph,
so a learning-rate schedule cannot reach a replay through them.  The update kernels therefore
read ``lr`` and ``weight_decay`` from this 16-byte device tensor, and :meth:`HyperBlock.set`
overwrites it between replays with one small async copy from pinned host memory.

* The device tensor is allocated at construction, before any capture, and never moves.
* The source rows live in a pinned table that is only ever appended to: a row that has been the
  source of a copy is never written again, so a copy still in flight always reads its own values.
  :meth:`prefill` writes the rows of a whole run ahead of time; :meth:`set` takes the next row
  (and writes it first only when it does not already hold the wanted pair).
* :meth:`set` enqueues nothing when the pair equals the last one uploaded: a constant schedule
  costs zero extra operations per step.
* The caller picks the stream (the copy goes on the current one): it must be the stream on which
  the update kernels that read the block are ordered — see :meth:`HyperState.set_hyper`.

:class:`HyperState` is the optimisers' side of it: ``lr`` / ``weight_decay`` / ``hyper`` /
``_hyper_on`` and the rules for changing them around a captured step, written once.
"""
from __future__ import annotations

import contextlib
from typing import Iterable, List, Optional, Tuple

import numpy as np
import torch

from . import capturing

__all__ = ["HyperBlock", "HyperState"]

_ROWS = 1024  # rows per pinned table when the run's length is not announced (16 KiB)


def _f32(v: float) -> float:
    return float(np.float32(v))


class HyperBlock:
    def __init__(self, device: torch.device, lr: float, weight_decay: float = 0.0):
        self.device = torch.device(device)
        assert self.device.type == "cuda", "the hyper block lives on the device (CPU twins read the floats)"
        self.last: Tuple[float, float] = (_f32(lr), _f32(weight_decay))
        self.dev = torch.tensor([self.last[0], self.last[1], 0.0, 0.0], dtype=torch.float32, device=self.device)
        self._tables: List[torch.Tensor] = []  # every pinned table so far (kept: a copy may be in flight)
        self._table: Optional[torch.Tensor] = None
        self._cur = 0     # next row of _table that has never been a copy source
        self._filled = 0  # rows [_cur, _filled) were written ahead by prefill()
        self.uploads = 0

    def _room(self, rows: int):
        """Make ``rows`` unused rows available at the cursor (a new table when the current one is short;
        the old one stays referenced)."""
        if self._table is not None and self._cur + rows <= self._table.shape[0]:
            return
        keep = self._table[self._cur: self._filled].clone() if self._table is not None else None
        self._table = torch.zeros(max(rows, _ROWS), 4, dtype=torch.float32).pin_memory()
        self._tables.append(self._table)
        n = 0 if keep is None else keep.shape[0]
        if n:
            self._table[:n].copy_(keep)
        self._cur, self._filled = 0, n

    def prefill(self, pairs: Iterable[Tuple[float, float]]):
        """Write the rows of the coming steps' ``(lr, weight_decay)`` pairs ahead of time: one row per
        change of value, in order, starting at the cursor (rows no copy has read yet)."""
        rows, prev = [], self.last
        for lr, wd in pairs:
            pair = (_f32(lr), _f32(wd))
            if pair != prev:
                rows.append(pair)
                prev = pair
        self._filled = self._cur  # rows written ahead earlier were never a copy source: overwritten
        self._room(len(rows))
        if rows:
            self._table[self._cur: self._cur + len(rows), :2] = torch.tensor(rows, dtype=torch.float32)
        self._filled = self._cur + len(rows)

    def set(self, lr: float, weight_decay: float, force: bool = False) -> bool:
        """Upload ``(lr, weight_decay)`` on the current stream unless it is what the block holds;
        returns whether a copy was enqueued."""
        pair = (_f32(lr), _f32(weight_decay))
        if pair == self.last and not force:
            return False
        assert not torch.cuda.is_current_stream_capturing(), "the hyper block is updated between replays"
        self._room(1)
        row = self._table[self._cur]
        if not (self._cur < self._filled and (float(row[0]), float(row[1])) == pair):
            row[0], row[1] = pair  # not written ahead: this row was never a copy source
        self.dev.copy_(row, non_blocking=True)
        self._cur += 1
        self._filled = max(self._filled, self._cur)
        self.last = pair
        self.uploads += 1
        return True


class HyperState:
    """Mixin of an optimiser whose update launches can read ``lr`` / ``weight_decay`` from a
    :class:`HyperBlock`: ``lr``, ``weight_decay`` (what a torch twin uses), ``hyper`` (the block, or
    None on CPU / without the native kernels: nothing is ever uploaded) and ``_hyper_on`` (the launches
    read the block; off, ``lr`` goes to them by value and there is no decay).

    Two hooks are all the variation between optimisers: :meth:`_hyper_on_side` and
    :meth:`_check_hyper`; ``_arm`` names the optimiser in error texts.
    """

    _arm = "optimiser"

    def _init_hyper(self, lr: float, weight_decay: float, block: bool, on: Optional[bool] = None):
        """``lr`` / ``weight_decay`` stored as given (the caller rounds, or does not).  ``block``: own a
        device block, allocated here, before any capture.  ``on``: whether the launches read it from
        the start (default: only with a decay; a kernel without a by-value ``lr`` passes True)."""
        self.lr, self.weight_decay = lr, weight_decay
        self.hyper = HyperBlock(self.device, lr, weight_decay) if block else None
        self._hyper_on = self.hyper is not None and (weight_decay != 0.0 if on is None else on)
        self._captured_by_value = False  # the last captured step froze lr into its graph
        self._captured_decay: Optional[bool] = None  # weight_decay != 0 when a step was last captured

    def _hyper_on_side(self) -> bool:
        """Hook: the launches that read the block run on the communicator's side stream."""
        return False

    def _check_hyper(self, lr: float, weight_decay: float) -> None:
        """Hook: an extra check (raise to refuse) before :meth:`set_hyper` accepts the fp32 values."""

    def _hyper_arg(self) -> Optional[torch.Tensor]:
        """The ``hyper=`` argument of this step's update launches (None: lr by value, no decay);
        inside a capture it records what the graph froze."""
        hy = self.hyper.dev if self._hyper_on else None
        if capturing():
            self._captured_by_value, self._captured_decay = hy is None, self.weight_decay != 0.0
        return hy

    def plan_hyper(self, pairs) -> None:
        """Write the pinned source rows of the coming steps' ``(lr, weight_decay)`` ahead of time."""
        if self.hyper is not None:
            self.hyper.prefill(pairs)

    def set_hyper(self, lr: float, weight_decay: Optional[float] = None) -> None:
        """Learning rate and weight decay of the steps from now on, captured replays included
        (``weight_decay=None`` keeps the current one).

        Both are rounded to fp32 once, kept in ``self.lr`` / ``self.weight_decay`` (what the torch
        twin uses) and, with a block, uploaded into it by one 16-byte async copy from a pinned row;
        nothing is enqueued when neither changed.  Never called inside a capture.  A step captured
        before the first call holds ``lr`` by value: changing what such a graph froze raises, and so
        does whatever :meth:`_check_hyper` refuses.

        Ordering of the copy: it must follow the previous step's last update launch and precede
        this step's first one.  When every launch of a step — eager or replayed — is on the
        current stream (no overlap groups, no stream mode), so is the copy.  With PowerSGD's overlap
        groups or the dense arm's stream mode the update launches run on the communicator's side
        stream; replayed, they sit at the tail of the comm graph, which is launched on that stream
        and is not joined with the current one between steps (a device flag, not the stream,
        releases the next compute graph), so a copy on the current stream could overtake them.  The
        copy therefore goes on the side stream itself (:meth:`_hyper_on_side`): stream order puts it
        after the previous comm graph (or eager side work) and before the next."""
        wd = self.weight_decay if weight_decay is None else float(weight_decay)
        assert wd >= 0, "weight_decay >= 0"
        lr, wd = _f32(lr), _f32(wd)
        if self._captured_by_value and (lr != _f32(self.lr) or wd != 0.0):
            raise RuntimeError(f"{self._arm}: the captured step holds lr by value; call set_hyper() before capturing")
        self._check_hyper(lr, wd)
        self.lr, self.weight_decay = lr, wd
        if self.hyper is not None:
            self._hyper_on = True
            self._upload_hyper()

    def _upload_hyper(self, force: bool = False) -> None:
        assert not capturing(), "set_hyper() inside a graph capture"
        with self.comm.on_side() if self._hyper_on_side() else contextlib.nullcontext():
            self.hyper.set(self.lr, self.weight_decay, force)

    def _load_hyper(self, lr: float, weight_decay: float) -> None:
        """The ``load_state_dict`` step: take the loaded values as given; the block follows them."""
        self.lr, self.weight_decay = lr, weight_decay
        if self.hyper is not None:
            self._hyper_on = self._hyper_on or weight_decay != 0.0
            self._upload_hyper(force=True)
