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
  the update kernels that read the block are ordered — see ``set_hyper`` of the optimisers.
"""
from __future__ import annotations

from typing import Iterable, List, Optional, Tuple

import numpy as np
import torch

__all__ = ["HyperBlock"]

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
