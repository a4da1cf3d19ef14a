"""Shapes and inputs of the AdamW kernel tests, shared by the CPU test (which checks that the inputs
tell the rule from its contracted variants) and the GPU test (which runs them).  numpy only."""
import numpy as np

from . import adamw_rule as R

F = np.float32
GUARD = 64            # floats around every gradient, parameter and moment
SEED = 20241021
SIZES = (1, 3, 4, 5, 1023, 2047, 2048, 2049, 4097)
ARMS = ((0, 0), (0, 1), (1, 0), (1, 1))   # (g, x) view start, floats past a 16-byte boundary
BIG = 270341          # 133 blocks of 2048: ticket groups of 64, 64 and 5
ONE_ENTRY = (64 * 2048, 64 * 2048 + 1)    # separate one-entry tables: 64 and 65 blocks
SENTINEL = F(-12345.678)
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
LR, WD = 1e-3, 0.05


def main_table():
    """[(numel, g_off, x_off, moment_off, decays)] of the one table: every size x alignment arm
    with the moments placed like the parameter (the FusedAdamW arrangement), two entries whose
    moments alone are misaligned (the float4 path needs all four streams), then the big entry;
    decaying and non-decaying entries alternate."""
    cases = [(n, a, b, b) for n in SIZES for a, b in ARMS] + [(5, 0, 0, 2), (2049, 0, 0, 3), (BIG, 0, 0, 0)]
    return [(n, a, b, c, i % 2 == 0) for i, (n, a, b, c) in enumerate(cases)]


def one_entry(n, decays=True):
    return [(n, 0, 0, 0, decays)]


def layout(cases, side):
    """Start (floats) of every tensor of ``cases`` in a flat 16-byte-aligned buffer of one ``side``
    (0: gradient, 1: parameter, 2: moments), GUARD floats free on both sides of each; returns
    (starts, total)."""
    starts, cur = [], 0
    for case in cases:
        pos = (cur + 3) // 4 * 4 + GUARD + case[1 + side]
        starts.append(pos)
        cur = pos + case[0] + GUARD
    return starts, (cur + 3) // 4 * 4


def buffers(cases, seed=SEED):
    """{"g", "x", "m", "v"}: (buffer, starts).  Gaussians in the gradients (scale 1e-2) and the
    parameters, zeros in the moments, SENTINEL in the guard bands."""
    out = {}
    for name, side in (("g", 0), ("x", 1), ("m", 2), ("v", 2)):
        starts, total = layout(cases, side)
        buf = np.full(total, SENTINEL, dtype=F)
        for i, (case, st) in enumerate(zip(cases, starts)):
            if name == "g":
                buf[st: st + case[0]] = R.gaussians(seed + i, case[0], 1e-2)
            elif name == "x":
                buf[st: st + case[0]] = R.gaussians(seed + 5000 + i, case[0])
            else:
                buf[st: st + case[0]] = F(0.0)
        out[name] = (buf, starts)
    return out


def next_grads(buf, cases, starts, k, seed=SEED):
    """The gradient buffer of launch ``k`` > 0: fresh Gaussians in the tensors, guards kept."""
    buf = buf.copy()
    for i, (case, st) in enumerate(zip(cases, starts)):
        buf[st: st + case[0]] = R.gaussians(seed + 100000 * k + i, case[0], 1e-2)
    return buf


def guard_mask(cases, starts, total):
    m = np.ones(total, dtype=bool)
    for case, st in zip(cases, starts):
        m[st: st + case[0]] = False
    return m


def specials():
    """(x, g, m, v) holding zeros of both signs, +-inf, NaN, 1e-20 (denormal squares), denormals
    and 1e25 (squares overflow), every gradient value against a few states."""
    inf, nan = np.inf, np.nan
    gv = [0.0, -0.0, 1e-20, -1e-20, 1e-38, 1e-42, 1e25, -1e25, inf, -inf, nan, 1.0, 3e-3]
    st = [(0.0, 0.0, 0.0), (-0.0, 0.0, 0.0), (1.5, 0.0, 0.0), (-2.0, 1e-3, 1e-6), (1.0, 1e-20, 1e-40),
          (1.0, -1e-20, 1e-44), (1.0, 1e20, 1e38), (inf, 0.0, 0.0), (1.0, inf, 1.0), (1.0, 1.0, inf), (nan, 0.0, 0.0)]
    rows = [(x, g, m, v) for g in gv for x, m, v in st]
    a = np.array(rows, dtype=F)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy(), a[:, 3].copy()
