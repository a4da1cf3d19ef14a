"""Shapes and inputs of the weight-EMA kernel tests, shared by the CPU test (which checks that the
inputs tell the rule from its fused variant) and the GPU test (which runs them).  numpy only."""
import numpy as np

from . import ema_rule as R

F = np.float32
GUARD = 64            # floats around every live tensor and every shadow
SEED = 20240611
SIZES = (1, 3, 4, 5, 1023, 2047, 2048, 2049, 4097)
ARMS = ((0, 0), (0, 1), (1, 0), (1, 1))   # (src, dst) view start, floats past a 16-byte boundary
BIG = 270341          # 133 blocks of 2048: ticket groups of 64, 64 and 5
ONE_ENTRY = (64 * 2048, 64 * 2048 + 1)    # separate one-entry tables: 64 and 65 blocks
SENTINEL = F(-12345.678)


def main_table():
    """[(numel, src_off, dst_off)] of the one table: every size x alignment arm, then the big entry."""
    return [(n, a, b) for n in SIZES for a, b in ARMS] + [(BIG, 0, 0)]


def layout(cases, side):
    """Start (floats) of every tensor of ``cases`` in a flat 16-byte-aligned buffer of one ``side``
    (0: live, 1: shadow), GUARD floats free on both sides of each; returns (starts, total)."""
    starts, cur = [], 0
    for case in cases:
        pos = (cur + 3) // 4 * 4 + GUARD + case[1 + side]
        starts.append(pos)
        cur = pos + case[0] + GUARD
    return starts, (cur + 3) // 4 * 4


def buffers(cases, seed=SEED):
    """(live buffer, shadow buffer, live starts, shadow starts): Gaussians in the tensors, SENTINEL
    in the guard bands."""
    out = []
    for side in (0, 1):
        starts, total = layout(cases, side)
        buf = np.full(total, SENTINEL, dtype=F)
        for i, (case, st) in enumerate(zip(cases, starts)):
            buf[st: st + case[0]] = R.gaussians(seed + 1000 * side + i, case[0])
        out.append((buf, starts))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def guard_mask(cases, starts, total):
    m = np.ones(total, dtype=bool)
    for case, st in zip(cases, starts):
        m[st: st + case[0]] = False
    return m
