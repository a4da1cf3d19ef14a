"""Learning-rate schedule: a pure function of the global step index and the config.

``s`` is the 0-based index of the step about to run; it continues across epochs and across a
resume, so a resumed run sees exactly the values of the uninterrupted one.  With

* ``S`` = steps per epoch, ``T = training_epochs * S`` = steps of the whole run,
* ``W = lr_warmup_steps``, ``base = learning_rate``:

=============  =====================================================================
``s < W``      ``base * (s + 1) / W``                                 (linear warm-up)
``constant``   ``base``
``step``       ``base * gamma**k``, ``k = #{milestones <= s // S}``   (milestones in epochs)
``cosine``     ``lr_min + (base - lr_min) * (1 + cos(pi (s - W) / (T - W))) / 2``
=============  =====================================================================

The value is evaluated in Python floats and rounded ONCE to fp32 (``numpy.float32``): that fp32
number is what the device block, the by-value kernel arguments and every torch twin use.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Sequence

import numpy as np

__all__ = ["LrSchedule", "parse_milestones", "SCHEDULES"]

SCHEDULES = ("constant", "step", "cosine")


def parse_milestones(text: str) -> List[int]:
    """``"15,25"`` -> ``[15, 25]``: increasing non-negative epochs (``ValueError`` otherwise)."""
    out = []
    for tok in (t.strip() for t in (text or "").split(",")):
        if not tok:
            continue
        if not tok.isdigit():
            raise ValueError(f"milestone {tok!r} is not a non-negative integer")
        out.append(int(tok))
    if any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError(f"milestones {out} are not increasing")
    return out


class LrSchedule:
    def __init__(self, base: float, steps_per_epoch: int, epochs: int, schedule: str = "constant",
                 warmup_steps: int = 0, lr_min: float = 0.0, milestones: Sequence[int] = (), gamma: float = 0.1):
        if schedule not in SCHEDULES:
            raise ValueError(f"lr_schedule {schedule!r}; allowed: {list(SCHEDULES)}")
        self.base = float(base)
        self.S = int(steps_per_epoch)
        self.T = int(epochs) * self.S
        self.schedule = schedule
        self.W = int(warmup_steps)
        self.lr_min = float(lr_min)
        self.milestones = list(milestones)
        self.gamma = float(gamma)
        if self.W and self.W >= self.T:
            raise ValueError(f"lr_warmup_steps {self.W} must be below the run's {self.T} steps")

    @classmethod
    def from_config(cls, config: Dict[str, Any], steps_per_epoch: int) -> "LrSchedule":
        return cls(config["learning_rate"], steps_per_epoch, config["training_epochs"],
                   schedule=config.get("lr_schedule", "constant"), warmup_steps=config.get("lr_warmup_steps", 0),
                   lr_min=config.get("lr_min", 0.0), milestones=parse_milestones(config.get("lr_milestones", "")),
                   gamma=config.get("lr_gamma", 0.1))

    @property
    def varies(self) -> bool:
        return self.schedule != "constant" or self.W > 0

    def lr_at(self, s: int) -> float:
        """The fp32 learning rate of step ``s`` (returned as a Python float: exactly that fp32 value)."""
        s = int(s)
        if s < self.W:
            lr = self.base * (s + 1) / self.W
        elif self.schedule == "step":
            k = sum(1 for e in self.milestones if e <= s // max(1, self.S))
            lr = self.base * self.gamma ** k
        elif self.schedule == "cosine":
            span = max(1, self.T - self.W)
            lr = self.lr_min + (self.base - self.lr_min) * 0.5 * (1.0 + math.cos(math.pi * (s - self.W) / span))
        else:
            lr = self.base
        return float(np.float32(lr))
