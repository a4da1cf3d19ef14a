"""The PowerSGD stage cases: every kernel instance the launchers of csrc/powersgd.hip can pick, at the
plan shapes (csrc/plan.cpp) where its code takes another path.  No extension, no GPU.

A Case is one plan -- matrix shapes, rank, the NDP_PSGD_PKW value the plan is built under (None: the
rank's default), the dead-tap supports (T, mask) per matrix, the bound-pointer misalignment per matrix
(floats past a 16-byte boundary) -- with the plan facts it claims as literals (columns per P item,
split-K chunks of P and Q, rows per Q item, compact columns, the kernel instance of each stage), and
the stage variants that tests/test_psgd_stages_gpu.py runs on it:

  p_vars  (fuse_ef, fused): fuse_ef "off" (M = g), "on" (M = g + e, stored), "prev" (lazy: M = g + e -
          P_prev Qs^T); fused: split-K finish and rank-1 pack in the launch, else p_out=None + seg_reduce
  q_vars  fused: split-K finish in the launch (matrices above Q_FIN_MAX chunks still by seg_reduce)
  u_vars  (mode, lazy, hyper, q_div, r1): hyper "none" (lr by value), "wd0" (block, wd = 0), "wd"
          (block, wd != 0); r1: elements of the rank-1 group stepped with the update (0: none)

tests/test_psgd_stage_cases_cpu.py pins the coverage from these literals and, with the extension
built, that build_plan reports the same facts.  Every matrix stays under 200k elements.

Shapes (P items are 16 x p_cols, wide; 64 x 256, narrow; Q items rc x 256; update tiles 16 x 256 / 64 x 64):
  wide sets, in units of the item width pc: (33, pc) one chunk, three row blocks, n % 16 = 1, q_off 0;
    (18, 9 pc + 12) 10 chunks: the 8-wide batch of chunk_sum_sc1 and a tail of 1; (5, 2 pc + 3) m % 4 != 0,
    r = min(n, R) below RQ; (9, 8 pc + 4) 9 chunks, bound 4 bytes off (vec = 0 at m % 4 == 0);
    (6, 18 pc + 4) 19 chunks: two batches and a tail of 2; (3, 7) n < 4, r = 3, odd m r so that the next
    q_off is unaligned; (16, 2 pc + 8) r % 4 == 0 at an unaligned q_off (q4 false).
  tall set: q_chunks 1, 2, 34 (last chunk 1 row, above Q_FIN_MAX), 61 (rc 68, last 17), 62 (rc 100, full),
    65 (rc 256); column blocks with inactive waves (m = 5, 300, 1030).
  narrow set: the same row counts at ranks above 16, m % 4 != 0, a bound 4 bytes off, 10 P chunks.
  taps set: T = 4 L = 1 (75 compact columns), T = 9 centre (130), {4,5,7,8} (64), 6 live (60), T = 16
    with 9 live (630: three column blocks, second taps word) and 15 live (120), one matrix without
    support, and two tapped ones with 3 and 34 Q row chunks.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

Q_FIN_MAX = 32          # parallel/powersgd.py: chunks the Q kernel's last arriver sums itself
R1_STRIDE = 131072      # elements one sweep of the update launch's rank-1 blocks covers (512 x 256)
MAX_ELEMS = 200_000


class Case(NamedTuple):
    name: str
    shapes: Tuple[Tuple[int, int], ...]
    rank: int
    pkw: Optional[int]
    supports: Optional[Tuple[Tuple[int, int], ...]]
    offs: Tuple[int, ...]
    # claimed plan facts
    p_cols: int
    p_chunks: Tuple[int, ...]
    q_chunks: Tuple[int, ...]
    q_rows: Tuple[int, ...]
    compact_cols: Tuple[int, ...]
    kernels: Tuple[str, str, str]  # P, Q, update instance
    # stage variants
    p_vars: tuple
    q_vars: tuple
    u_vars: tuple

    @property
    def ranks(self):
        return tuple(min(n, m, self.rank) for n, m in self.shapes)

    @property
    def max_rank(self):
        return max(self.ranks)

    @property
    def wide(self):
        return self.max_rank <= 16

    def support(self, i):
        """(T, mask) of matrix i where the plan compacts it, else None"""
        return self.supports[i] if self.compact_cols[i] != self.shapes[i][1] else None


WIDE_SETS = {
    256: ((33, 256), (18, 2316), (5, 515), (9, 2052), (6, 4612), (3, 7), (16, 520)),
    512: ((33, 512), (18, 4620), (5, 1027), (9, 4100), (6, 9220), (3, 7), (16, 1032)),
    1024: ((33, 1024), (18, 9228), (5, 2051), (9, 8196), (6, 18436), (3, 7), (16, 2056)),
}
WIDE_OFFS = (0, 0, 0, 1, 0, 0, 0)
TALL = ((64, 300), (65, 5), (2113, 12), (4097, 12), (6200, 8), (16400, 6), (40, 1030))
NARROW = ((4097, 40), (2113, 33), (65, 300), (16400, 12), (40, 1030), (70, 45), (36, 64), (6200, 20), (40, 2310))
# rank 40: one MGS workgroup per 256 rows and at most 64 of them without a device, so 16380 rows (rc still 256)
NARROW_40 = NARROW[:3] + ((16380, 12),) + NARROW[4:]
NARROW_OFFS = (0, 0, 0, 0, 0, 0, 1, 0, 0)
TAPS = ((20, 300), (18, 1170), (18, 144), (33, 90), (17, 1120), (5, 128), (12, 40), (130, 72), (2113, 12))
TAP_SUPPORTS = ((4, 0b0100), (9, 1 << 4), (9, 0b110110000), (9, 0b110110110), (16, 0x0FF8), (16, 0xFFBF), (0, 0),
                (9, 1 << 4), (4, 0b0100))
TAP_COMPACT = (75, 130, 64, 60, 630, 120, 40, 8, 3)

P_ALL = (("off", True), ("on", True), ("prev", True), ("on", False))
U_WIDE = ((0, False, "none", 1, 0), (1, False, "none", 4, 300), (1, True, "wd0", 1, 1),
          (2, False, "wd", 4, R1_STRIDE + 300), (2, True, "wd", 1, 300), (3, False, "none", 4, 0))
U_TALL = ((1, False, "none", 4, 300), (2, True, "wd", 1, 0))
U_NARROW = ((0, False, "none", 1, 0), (1, False, "wd0", 4, 300), (2, False, "wd", 4, R1_STRIDE + 300))
# the compact update tile takes no decay (the engine keeps every matrix full under weight decay)
U_TAPS = ((1, False, "none", 4, 300), (1, True, "wd0", 1, 1), (2, False, "none", 1, 0), (2, True, "wd0", 4, 0),
          (3, False, "none", 4, 0))


def _wide(rank, pc, default):
    return Case(
        name=f"wide-r{rank}-pkw{pc}" + ("-default" if default else ""),
        shapes=WIDE_SETS[pc], rank=rank, pkw=None if default else pc, supports=None, offs=WIDE_OFFS,
        p_cols=pc, p_chunks=(1, 10, 3, 9, 19, 1, 3), q_chunks=(1, 1, 1, 1, 1, 1, 1), q_rows=(33, 18, 5, 9, 6, 3, 16),
        compact_cols=tuple(m for _, m in WIDE_SETS[pc]),
        kernels=(f"p_wide<{rank},{pc}>", "q<1>", f"update_wide<{rank}>"),
        p_vars=P_ALL, q_vars=(True, False) if default else (), u_vars=U_WIDE if default else ())


def _tall(rank, pc, p_chunks):
    return Case(
        name=f"tall-r{rank}", shapes=TALL, rank=rank, pkw=None, supports=None, offs=(0,) * 7,
        p_cols=pc, p_chunks=p_chunks, q_chunks=(1, 2, 34, 61, 62, 65, 1), q_rows=(64, 64, 64, 68, 100, 256, 40),
        compact_cols=tuple(m for _, m in TALL), kernels=(f"p_wide<{rank},{pc}>", "q<1>", f"update_wide<{rank}>"),
        p_vars=(("on", True), ("prev", True)), q_vars=(True, False), u_vars=U_TALL)


def _narrow(rank, ncg, shapes, q_chunks):
    return Case(
        name=f"narrow-r{rank}", shapes=shapes, rank=rank, pkw=None, supports=None, offs=NARROW_OFFS,
        p_cols=256, p_chunks=(1, 1, 2, 1, 5, 1, 1, 1, 10), q_chunks=q_chunks,
        q_rows=(68, 64, 64, 256, 40, 64, 36, 100, 40), compact_cols=tuple(m for _, m in shapes),
        kernels=(f"p<{ncg}>", f"q<{ncg}>", "update"),
        p_vars=(("off", False), ("on", False)), q_vars=(False,), u_vars=U_NARROW)


def _taps(rank, pkw, pc, p_chunks):
    return Case(
        name=f"taps-r{rank}" + (f"-pkw{pkw}" if pkw else ""), shapes=TAPS, rank=rank, pkw=pkw,
        supports=TAP_SUPPORTS, offs=(0,) * 9,
        p_cols=pc, p_chunks=p_chunks, q_chunks=(1, 1, 1, 1, 1, 1, 1, 3, 34), q_rows=(20, 18, 18, 33, 17, 5, 12, 64, 64),
        compact_cols=TAP_COMPACT, kernels=(f"p_wide<{rank},{pc}>", "q<1>", f"update_wide<{rank}>"),
        p_vars=P_ALL, q_vars=(True, False), u_vars=U_TAPS)


CASES = (
    _wide(4, 256, False), _wide(4, 512, True), _wide(4, 1024, False),
    _wide(8, 256, False), _wide(8, 512, True), _wide(8, 1024, False),
    _wide(16, 256, False), _wide(16, 512, False), _wide(16, 1024, True),
    _tall(4, 512, (1, 1, 1, 1, 1, 1, 3)), _tall(16, 1024, (1, 1, 1, 1, 1, 1, 2)),
    _narrow(24, 2, NARROW, (61, 34, 2, 65, 1, 2, 1, 62, 1)), _narrow(40, 4, NARROW_40, (61, 34, 2, 64, 1, 2, 1, 62, 1)),
    _taps(4, None, 512, (1, 3, 1, 1, 3, 1, 1, 1, 1)),
    _taps(8, 1024, 1024, (1, 2, 1, 1, 2, 1, 1, 1, 1)),
    _taps(16, None, 1024, (1, 2, 1, 1, 2, 1, 1, 1, 1)),
)
RANK1_SIZES = (1, 300, R1_STRIDE + 300)  # rank1_step on its own: one thread, a partial block, the grid-stride loop


def instances(max_rank: int, p_cols: int) -> Tuple[str, str, str]:
    """the (P, Q, update) kernel instances launch_psgd_p / _q / _update pick for a plan"""
    c = (max_rank + 15) // 16
    ncg = 1 if c <= 1 else 2 if c == 2 else 4
    if max_rank <= 16:
        rq = 4 if max_rank <= 4 else 8 if max_rank <= 8 else 16
        return f"p_wide<{rq},{p_cols}>", f"q<{ncg}>", f"update_wide<{rq}>"
    return f"p<{ncg}>", f"q<{ncg}>", "update"


def by_name(name: str) -> Case:
    return next(c for c in CASES if c.name == name)


def stage_runs():
    """(stage, case, variant) of every GPU run, per input arm"""
    out = []
    for c in CASES:
        out += [("p", c, v) for v in c.p_vars] + [("q", c, v) for v in c.q_vars] + [("u", c, v) for v in c.u_vars]
    return out


def chunk_sum_tail(chunks: int) -> Tuple[int, int]:
    """(8-wide batches, tail length) chunk_sum_sc1 runs for a split of ``chunks`` (the first chunk is
    loaded on its own)"""
    return (chunks - 1) // 8, (chunks - 1) % 8
