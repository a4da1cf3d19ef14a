"""The tgemm cases: every kernel instance launch_tile of csrc/tgemm.hip can reach through tg_fwd /
tg_dgrad / tg_wgrad, at the launch shapes where the kernel takes another path.  No extension, no GPU.

A Case is one launch: the conv (B, C, H, W, Co) (1x1, stride 1), the direction, the bytes the base
pointers of the A and B operands sit past a 16-byte boundary (0 or 4; A / B are w / x in forward,
w / dy in grad-x, dy / x in grad-W), whether grad-x adds an addend in place, whether the split-K
slabs are left to the caller (defer) -- and the facts it claims as literals: the instance
tgemm_kernel<64,64,32, AKF, BNF, WA, WB, 2> as "TT44" .. "FF11", the GEMM M, N, K, the slabs
tg_splits allots (splits) and the slabs run() launches after rounding a split to whole k-tiles
(slabs).  tests/test_tg_cases_cpu.py pins the coverage from these literals and, with the extension
built, that tg_describe reports the same facts for every case and that no instance reachable on its
sweep grid is missing; tests/test_tg_instances_gpu.py runs each Case.

What selects an instance (tg_args, vec_ok):
  forward  AKF always; BNF iff the map has >= 4 pixels; WA = 4 iff C % 4 == 0 and w is aligned; WB = 4
           iff BNF and x is aligned
  grad-x   AKF never; BNF, WB as forward (dy for x); WA = 4 iff C % 4 == 0 and w is aligned
  grad-W   BNF never; AKF iff the map has >= 4 pixels; WA = 4 iff AKF and dy is aligned; WB = 4 iff AKF
           and x is aligned
which is 6 + 6 + 5 = 17 (direction, instance) pairs over 14 instances; FT.. on a 2-pixel map and
TT.. / FT.. in grad-W do not occur.

Launch shapes.  The k loop runs in rounds of two k-tiles plus a tail, after a two-tile prologue, so
1 .. 5 k-tiles per split walk every phase of it.  tg_pick_splits doubles the split count s while the
K range holds at least 4 s k-tiles (up to 4 slabs in forward and grad-x, 64 in grad-W, and 256
workgroups in all), so a split holds 2 .. 4 k-tiles until a cap binds: 5 per split needs >= 16 k-tiles
in forward / grad-x (C or Co of 548 here) and, in grad-W, K > 8192 or >= 128 output tiles -- operands
of megabytes, so grad-W stops at 4 here (PER_SPLIT).  Every tensor stays under MAX_ELEMS floats.
"""
from __future__ import annotations

from typing import NamedTuple, Tuple

FWD, DGRAD, WGRAD = 0, 1, 2
DIR_NAMES = ("fwd", "dgrad", "wgrad")
BK = 32                 # csrc/tgemm.hip kTile64: k-tile depth; the tile is 64 x 64
MAX_ELEMS = 100_000     # floats per tensor (400 kB)


class Case(NamedTuple):
    name: str
    shape: Tuple[int, int, int, int, int]  # B, C, H, W, Co
    dir: int
    a_off: int      # bytes past 16-B alignment of operand A's base
    b_off: int      # ... of operand B's
    addend: bool    # grad-x only: dx = grad-x + addend, written over the addend
    defer: bool
    # claimed facts
    instance: str
    M: int
    N: int
    K: int
    splits: int
    slabs: int

    @property
    def geom(self):
        _B, C, H, W, Co = self.shape
        return [C, H, W, Co, 1, 1, 1, 0]

    @property
    def B(self):
        return self.shape[0]

    @property
    def ktiles(self):
        return -(-self.K // BK)

    @property
    def per(self):
        """k-tiles per split, as run() rounds them"""
        return -(-self.ktiles // self.splits)

    @property
    def kchunk(self):
        return self.per * BK

    @property
    def pair(self):
        return (self.dir, self.instance)

    def sizes(self):
        """floats in x, w, y"""
        B, C, H, W, Co = self.shape
        return B * C * H * W, Co * C, B * Co * H * W


CASES = (
    # ---- forward: M = Co, N = B hw, K = C; A = w, B = x
    Case("fwd-tiny-c6", (2, 6, 2, 2, 4), FWD, 0, 0, False, False, "TT14", 4, 8, 6, 1, 1),
    Case("fwd-tiny-c6-xoff", (2, 6, 2, 2, 4), FWD, 0, 4, False, False, "TT11", 4, 8, 6, 1, 1),
    Case("fwd-1x2", (2, 8, 1, 2, 4), FWD, 0, 0, False, False, "TF41", 4, 4, 8, 1, 1),
    Case("fwd-1x2-woff", (2, 8, 1, 2, 4), FWD, 4, 0, False, False, "TF11", 4, 4, 8, 1, 1),
    Case("fwd-2x1-c6", (2, 6, 2, 1, 4), FWD, 0, 0, False, False, "TF11", 4, 4, 6, 1, 1),
    Case("fwd-2x1-c70", (2, 70, 2, 1, 4), FWD, 0, 0, False, False, "TF11", 4, 4, 70, 1, 1),
    Case("fwd-1x2-split2", (2, 128, 1, 2, 4), FWD, 0, 0, False, False, "TF41", 4, 4, 128, 2, 2),
    Case("fwd-c18", (4, 18, 4, 4, 20), FWD, 0, 0, False, False, "TT14", 20, 64, 18, 1, 1),
    Case("fwd-ragged", (6, 36, 4, 4, 40), FWD, 0, 0, False, False, "TT44", 40, 96, 36, 1, 1),
    Case("fwd-ragged-xoff", (6, 36, 4, 4, 40), FWD, 0, 4, False, False, "TT41", 40, 96, 36, 1, 1),
    Case("fwd-ragged-woff", (6, 36, 4, 4, 40), FWD, 4, 0, False, False, "TT14", 40, 96, 36, 1, 1),
    Case("fwd-ragged-c38-xoff", (6, 38, 4, 4, 40), FWD, 0, 4, False, False, "TT11", 40, 96, 38, 1, 1),
    Case("fwd-m64-k96", (3, 96, 4, 4, 64), FWD, 0, 0, False, False, "TT44", 64, 48, 96, 1, 1),
    Case("fwd-m68-split2", (2, 100, 8, 8, 68), FWD, 0, 0, False, False, "TT44", 68, 128, 100, 2, 2),
    Case("fwd-m68-split2-defer", (2, 100, 8, 8, 68), FWD, 0, 0, False, True, "TT44", 68, 128, 100, 2, 2),
    Case("fwd-split4", (2, 256, 2, 2, 8), FWD, 0, 0, False, False, "TT44", 8, 8, 256, 4, 4),
    Case("fwd-split4-short", (2, 260, 2, 2, 8), FWD, 0, 0, False, False, "TT44", 8, 8, 260, 4, 3),
    Case("fwd-split4-short-defer", (2, 260, 2, 2, 8), FWD, 0, 0, False, True, "TT44", 8, 8, 260, 4, 3),
    Case("fwd-per4", (2, 200, 2, 2, 8), FWD, 0, 0, False, False, "TT44", 8, 8, 200, 2, 2),
    Case("fwd-per5", (2, 548, 2, 2, 8), FWD, 0, 0, False, False, "TT44", 8, 8, 548, 4, 4),
    # ---- grad-x: M = C, N = B hw, K = Co; A = w, B = dy
    Case("dgrad-tiny-c6", (2, 6, 2, 2, 4), DGRAD, 0, 0, False, False, "FT14", 6, 8, 4, 1, 1),
    Case("dgrad-tiny-c6-dyoff", (2, 6, 2, 2, 4), DGRAD, 0, 4, False, False, "FT11", 6, 8, 4, 1, 1),
    Case("dgrad-1x2", (2, 8, 1, 2, 4), DGRAD, 0, 0, False, False, "FF41", 8, 4, 4, 1, 1),
    Case("dgrad-1x2-woff", (2, 8, 1, 2, 4), DGRAD, 4, 0, False, False, "FF11", 8, 4, 4, 1, 1),
    Case("dgrad-2x1-c6", (2, 6, 2, 1, 4), DGRAD, 0, 0, False, False, "FF11", 6, 4, 4, 1, 1),
    Case("dgrad-2x1-c6-k70-add", (2, 6, 2, 1, 70), DGRAD, 0, 0, True, False, "FF11", 6, 4, 70, 1, 1),
    Case("dgrad-1x2-split2", (2, 4, 1, 2, 128), DGRAD, 0, 0, False, False, "FF41", 4, 4, 128, 2, 2),
    Case("dgrad-c18-add", (4, 18, 4, 4, 20), DGRAD, 0, 0, True, False, "FT14", 18, 64, 20, 1, 1),
    Case("dgrad-ragged", (6, 40, 4, 4, 36), DGRAD, 0, 0, False, False, "FT44", 40, 96, 36, 1, 1),
    Case("dgrad-ragged-add", (6, 40, 4, 4, 36), DGRAD, 0, 0, True, False, "FT44", 40, 96, 36, 1, 1),
    Case("dgrad-ragged-dyoff", (6, 40, 4, 4, 36), DGRAD, 0, 4, False, False, "FT41", 40, 96, 36, 1, 1),
    Case("dgrad-ragged-woff", (6, 40, 4, 4, 36), DGRAD, 4, 0, False, False, "FT14", 40, 96, 36, 1, 1),
    Case("dgrad-ragged-c38-dyoff-add", (6, 38, 4, 4, 40), DGRAD, 0, 4, True, False, "FT11", 38, 96, 40, 1, 1),
    Case("dgrad-m64-k96", (3, 64, 4, 4, 96), DGRAD, 0, 0, False, False, "FT44", 64, 48, 96, 1, 1),
    Case("dgrad-m68-add", (2, 68, 8, 8, 36), DGRAD, 0, 0, True, False, "FT44", 68, 128, 36, 1, 1),
    Case("dgrad-m68-split2", (2, 68, 8, 8, 100), DGRAD, 0, 0, False, False, "FT44", 68, 128, 100, 2, 2),
    Case("dgrad-m68-split2-defer", (2, 68, 8, 8, 100), DGRAD, 0, 0, False, True, "FT44", 68, 128, 100, 2, 2),
    Case("dgrad-m68-split2-add", (2, 68, 8, 8, 100), DGRAD, 0, 0, True, False, "FT44", 68, 128, 100, 2, 2),
    Case("dgrad-split4", (2, 8, 2, 2, 256), DGRAD, 0, 0, False, False, "FT44", 8, 8, 256, 4, 4),
    Case("dgrad-split4-short-add", (2, 8, 2, 2, 260), DGRAD, 0, 0, True, False, "FT44", 8, 8, 260, 4, 3),
    Case("dgrad-split4-short-defer", (2, 8, 2, 2, 260), DGRAD, 0, 0, False, True, "FT44", 8, 8, 260, 4, 3),
    Case("dgrad-per4", (2, 8, 2, 2, 200), DGRAD, 0, 0, False, False, "FT44", 8, 8, 200, 2, 2),
    Case("dgrad-per5", (2, 8, 2, 2, 548), DGRAD, 0, 0, False, False, "FT44", 8, 8, 548, 4, 4),
    # ---- grad-W: M = Co, N = C, K = B hw; A = dy, B = x
    Case("wgrad-tiny", (2, 6, 2, 2, 4), WGRAD, 0, 0, False, False, "TF44", 4, 6, 8, 1, 1),
    Case("wgrad-tiny-xoff", (2, 6, 2, 2, 4), WGRAD, 0, 4, False, False, "TF41", 4, 6, 8, 1, 1),
    Case("wgrad-tiny-dyoff", (2, 6, 2, 2, 4), WGRAD, 4, 0, False, False, "TF14", 4, 6, 8, 1, 1),
    Case("wgrad-tiny-bothoff", (2, 6, 2, 2, 4), WGRAD, 4, 4, False, False, "TF11", 4, 6, 8, 1, 1),
    Case("wgrad-1x2", (2, 8, 1, 2, 4), WGRAD, 0, 0, False, False, "FF11", 4, 8, 4, 1, 1),
    Case("wgrad-2x1-k70", (35, 6, 2, 1, 4), WGRAD, 0, 0, False, False, "FF11", 4, 6, 70, 1, 1),
    Case("wgrad-1x2-split2", (64, 8, 1, 2, 4), WGRAD, 0, 0, False, False, "FF11", 4, 8, 128, 2, 2),
    Case("wgrad-c18", (4, 18, 4, 4, 20), WGRAD, 0, 0, False, False, "TF44", 20, 18, 64, 1, 1),
    Case("wgrad-ragged", (6, 36, 4, 4, 40), WGRAD, 0, 0, False, False, "TF44", 40, 36, 96, 1, 1),
    Case("wgrad-ragged-xoff", (6, 36, 4, 4, 40), WGRAD, 0, 4, False, False, "TF41", 40, 36, 96, 1, 1),
    Case("wgrad-ragged-dyoff", (6, 36, 4, 4, 40), WGRAD, 4, 0, False, False, "TF14", 40, 36, 96, 1, 1),
    Case("wgrad-ragged-bothoff", (6, 36, 4, 4, 40), WGRAD, 4, 4, False, False, "TF11", 40, 36, 96, 1, 1),
    Case("wgrad-m64-k48", (3, 64, 4, 4, 64), WGRAD, 0, 0, False, False, "TF44", 64, 64, 48, 1, 1),
    Case("wgrad-m72-split2", (2, 68, 8, 8, 72), WGRAD, 0, 0, False, False, "TF44", 72, 68, 128, 2, 2),
    Case("wgrad-m72-split2-defer", (2, 68, 8, 8, 72), WGRAD, 0, 0, False, True, "TF44", 72, 68, 128, 2, 2),
    Case("wgrad-per4", (13, 8, 4, 4, 4), WGRAD, 0, 0, False, False, "TF44", 4, 8, 208, 2, 2),
    # 33 k-tiles: 16 slabs allotted, 3 k-tiles each, so 11 launched; the last holds 96 / 84 of K
    Case("wgrad-k1056", (66, 64, 4, 4, 64), WGRAD, 0, 0, False, False, "TF44", 64, 64, 1056, 16, 11),
    Case("wgrad-k1056-defer", (66, 64, 4, 4, 64), WGRAD, 0, 0, False, True, "TF44", 64, 64, 1056, 16, 11),
    Case("wgrad-k1044", (261, 8, 2, 2, 4), WGRAD, 0, 0, False, False, "TF44", 4, 8, 1044, 16, 11),
    Case("wgrad-k1044-defer-bothoff", (261, 8, 2, 2, 4), WGRAD, 4, 4, False, True, "TF11", 4, 8, 1044, 16, 11),
)

# every (direction, instance) pair the dispatch can reach
PAIRS = frozenset(
    [(FWD, i) for i in ("TT44", "TT14", "TT41", "TT11", "TF41", "TF11")]
    + [(DGRAD, i) for i in ("FT44", "FT14", "FT41", "FT11", "FF41", "FF11")]
    + [(WGRAD, i) for i in ("TF44", "TF14", "TF41", "TF11", "FF11")])

# k-tiles per split each direction must show (module docstring: grad-W stops at 4)
PER_SPLIT = {FWD: (1, 2, 3, 4, 5), DGRAD: (1, 2, 3, 4, 5), WGRAD: (1, 2, 3, 4)}

# the sweep of tests/test_tg_cases_cpu.py
SWEEP_CHANNELS = (4, 6, 8, 18, 20, 36, 64, 68)
SWEEP_MAPS = ((1, 2), (2, 1), (2, 2), (4, 4), (8, 8))
SWEEP_BATCHES = (2, 4, 6, 66)
SWEEP_OFFS = ((0, 0), (0, 4), (4, 0), (4, 4))


def instance_name(d) -> str:
    """"TT44" .. "FF11" of a tg_describe dict"""
    return ("T" if d["akf"] else "F") + ("T" if d["bnf"] else "F") + f"{d['wa']}{d['wb']}"


def by_name(name: str) -> Case:
    return next(c for c in CASES if c.name == name)
