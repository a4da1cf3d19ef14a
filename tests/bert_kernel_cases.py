"""The DistilBERT kernel cases: every template instance and launch geometry of csrc/layernorm.hip,
csrc/attention.hip, csrc/linear.hip and csrc/embedding.hip, at the smallest shapes that reach them.  Pure
Python on top of tests/bert_rule.py: no extension, no GPU.  tests/test_bert_kernel_cases_cpu.py pins that
nothing is left out and that the geometry twins give what each class claims;
tests/test_bert_kernels_gpu.py runs each case through the bindings.

LayerNorm (LnCase).  LN_SWITCH builds <V, DM> for D = 256 V in {256, 512, 768, 1024} and dropout mode DM
in {0, 1, 2}, forward and backward; a case runs both.  Row classes: R = 1 (one live wave), 3 (a partial
workgroup), 9 (three workgroups, the last with one row) and 2051: ln_bwd_wgs caps at 512 workgroups, so
rows_per_wave is 2, waves past row 2051 are idle and wave 1025 holds the single row 2050.  Every
(D, mode) runs once more with part_out (deferred) at R = 2051, and D = 768 also at R = 3 (a single
slab).  p = 0.1 everywhere.

Attention (AttnCase).  Mask patterns, on batch row 0 unless noted:
  none    no mask
  tail    keys from 2 S // 3 on are masked: a tail that starts inside a key block
  first   keys 0..63 masked (a skipped first block)
  middle  keys 64..127 masked (a skipped middle block)
  padded  batch row 1 fully padded, S = 129: three key blocks, row_any false, nothing skipped, HF's
          uniform average; row 0 carries the tail
  long    S = 4160: keys 128..191 masked (a skipped block inside the 64-entry map) and keys 4100..4159
          masked, so that block 64 (keys 4096..4159) holds attended and masked keys, lies outside the map
          and is never skipped

Threshold-gap cases.  An element whose hash lies in [thr64(p), thr32(p)) is kept under the double
threshold and dropped under the fp32 one the attention launchers used to compute.  The seeds below are
the first that search_attn_gap / search_ln_gap find from seed 0 at the case's shape (seconds on a CPU;
the CPU test starts each search one below the literal, and checks the named element's hash).  The
attention cases pin the fix, the LayerNorm cases that ln_drop stays on the double threshold.

Column sums and GELU backward (ColCase): N in {4, 132, 256, 260, 768} (one lane, a partial strip, a full
strip, a second strip with one live lane, three strips) x M in {1, 5, 31, 32, 33, 100}, the M at which
every lane group of the chunk adds exactly 3, 4 and 5 rows (tail only / one unrolled step / unrolled step
and tail; derived from the twin), and (32768, 4), which reaches the 1024-chunk cap.

Embedding (EmbCase): T on both sides of the 64-id step and of the 8192-id tile, V = 1 and 5 (partial
workgroups of the gather), D = 260 (a second pass of the 64-lane column loop); every value of every axis
appears, not every combination.
"""
from __future__ import annotations

import itertools
from typing import NamedTuple, Optional, Tuple

import torch

from tests import bert_rule as R

P = 0.1
SEED = 987654          # the seed of tests/test_layernorm_gpu.py
NEG_SEED = -987654     # (uint32_t) of a negative int32

# ------------------------------------------------ LayerNorm ------------------------------------------------
LN_D = (256, 512, 768, 1024)
LN_MODES = (0, 1, 2)
LN_ROWS = (1, 3, 9, 2051)
LN_GAP = dict(p=0.1, R=2051, D=768, seed=337, row=1918, col=109)


class LnCase(NamedTuple):
    id: str
    D: int
    mode: int
    res: bool
    R: int
    deferred: bool
    p: float
    seed: int
    gap: Optional[Tuple[int, int]]   # (row, col) whose hash lies in [thr64(p), thr32(p))

    @property
    def instance(self):
        return (self.D // 256, self.mode)


def _ln(D, mode, res, Rr, deferred=False, seed=SEED, gap=None, tag=""):
    cid = f"D{D}-mode{mode}-{'res' if res else 'nores'}-R{Rr}" + ("-deferred" if deferred else "") + tag
    return LnCase(cid, D, mode, res, Rr, deferred, P, seed, gap)


def ln_cases():
    out = [_ln(D, m, res, Rr) for D, m, res, Rr in itertools.product(LN_D, LN_MODES, (False, True), LN_ROWS)]
    out += [_ln(D, m, True, 2051, deferred=True) for D, m in itertools.product(LN_D, LN_MODES)]
    out += [_ln(768, m, True, 3, deferred=True) for m in LN_MODES]
    out += [_ln(768, 1, True, 9, seed=NEG_SEED, tag="-negseed")]
    g = LN_GAP
    out += [_ln(g["D"], m, True, g["R"], seed=g["seed"], gap=(g["row"], g["col"]), tag="-gap") for m in (1, 2)]
    return out


def search_ln_gap(p, Rr, D, start=0):
    """the first seed >= start with an element of [Rr, D] whose ln_hash lies in [thr64(p), thr32(p)), and
    that element"""
    lo, hi = R.thr64(p), R.thr32(p)
    r = torch.arange(Rr, dtype=torch.int64).view(-1, 1)
    c = torch.arange(D, dtype=torch.int64).view(1, -1)
    for seed in itertools.count(start):
        h = R.ln_hash(seed, r, c)
        hit = torch.nonzero((h >= lo) & (h < hi))
        if hit.numel():
            return seed, tuple(hit[0].tolist())


# ------------------------------------------------ attention ------------------------------------------------
ATTN_S = (1, 5, 63, 64, 65, 129, 200)
ATTN_H = (1, 3)
ATTN_PATTERNS = ("none", "tail", "first", "middle", "padded", "long")
LONG_S = 4160
# p, seed, (bh, query, key): B * H = 2, S = 80, unmasked
ATTN_GAPS = ((0.1, 55741, (0, 53, 51)), (0.2, 5351, (0, 64, 54)), (0.3, 1811, (0, 1, 29)))
GAP_S = 80


class AttnCase(NamedTuple):
    id: str
    B: int
    S: int
    H: int
    pattern: str
    p: float
    seed: int
    packed: bool                         # q / k / v (and their gradients) views into [B, S, 3, H, 64]
    gap: Optional[Tuple[int, int, int]]  # (bh, query, key) whose hash lies in [thr64(p), thr32(p))


def _at(B, S, H, pattern, p=0.0, seed=12345, packed=False, gap=None, tag=""):
    cid = f"B{B}-S{S}-H{H}-{pattern}-p{p}" + ("-packed" if packed else "") + tag
    return AttnCase(cid, B, S, H, pattern, p, seed, packed, gap)


def attn_cases():
    out = [
        _at(2, 1, 1, "none"), _at(2, 1, 3, "none", P, packed=True),
        _at(2, 5, 3, "tail"), _at(2, 5, 1, "none", P),
        _at(2, 63, 1, "tail", P, packed=True), _at(2, 63, 3, "none"),
        _at(2, 64, 3, "none"), _at(2, 64, 1, "tail", P),
        _at(2, 65, 1, "tail"), _at(2, 65, 3, "none", P, packed=True),
        _at(2, 129, 1, "first"), _at(2, 129, 3, "padded"), _at(2, 129, 3, "padded", P),
        _at(2, 200, 1, "middle", P), _at(2, 200, 3, "first", P, packed=True), _at(2, 200, 1, "tail", packed=True),
        _at(2, 65, 3, "tail", P, seed=-12345, tag="-negseed"),
        _at(1, LONG_S, 1, "long"),
    ]
    out += [_at(1, GAP_S, 2, "none", p, seed, gap=g, tag="-gap") for p, seed, g in ATTN_GAPS]
    return out


def attn_mask(case):
    """[B][S] of 0 / 1, or None"""
    B, S = case.B, case.S
    if case.pattern == "none":
        return None
    m = [[1] * S for _ in range(B)]

    def zero(b, lo, hi):
        for i in range(lo, hi):
            m[b][i] = 0

    if case.pattern in ("tail", "padded"):
        zero(0, 2 * S // 3, S)
    if case.pattern == "padded":
        zero(1, 0, S)
    if case.pattern == "first":
        zero(0, 0, 64)
    if case.pattern == "middle":
        zero(0, 64, 128)
    if case.pattern == "long":
        zero(0, 128, 192)
        zero(0, 4100, 4160)
    return m


def search_attn_gap(p, BH, S, start=0):
    """the first seed >= start with an element of [BH, S, S] whose attn_hash lies in [thr64(p), thr32(p)),
    and that element"""
    lo, hi = R.thr64(p), R.thr32(p)
    ar = lambda n, shape: torch.arange(n, dtype=torch.int64).view(shape)  # noqa: E731
    bh, q, k = ar(BH, (-1, 1, 1)), ar(S, (1, -1, 1)), ar(S, (1, 1, -1))
    for seed in itertools.count(start):
        h = R.attn_hash(seed, bh, q, k)
        hit = torch.nonzero((h >= lo) & (h < hi))
        if hit.numel():
            return seed, tuple(hit[0].tolist())


# ---------------------------------------- column sums, GELU backward ---------------------------------------
COL_N = (4, 132, 256, 260, 768)
COL_M = (1, 5, 31, 32, 33, 100)
COL_GROUP_ROWS = (3, 4, 5)   # rows per lane group around the 4-row unrolled step
BOUNDARY_N = 260
CAP_MN = (32768, 4)
# the special inputs that lead GELU's h, before the random fill (g stays random there)
GELU_SPECIALS = (0.0, -0.0, 1e-30, -1e-30, 0.5, -0.5, 3.0, -3.0, 10.0, -10.0, 40.0, -40.0)


class ColCase(NamedTuple):
    id: str
    M: int
    N: int


def boundary_m(n, N=BOUNDARY_N):
    """the smallest M at which every lane group of the (single) chunk adds exactly n rows"""
    for M in itertools.count(1):
        if R.group_rows(M, N) == [[n] * 4]:
            return M


def col_cases():
    mn = [(M, N) for N in COL_N for M in COL_M]
    mn += [(boundary_m(n), BOUNDARY_N) for n in COL_GROUP_ROWS]
    mn += [CAP_MN]
    return [ColCase(f"M{M}-N{N}", M, N) for M, N in mn]


# ------------------------------------------------ embedding ------------------------------------------------
EMB_T = (0, 1, 63, 64, 65, 300, 8191, 8192, 8193)
EMB_V = (1, 5, 97)
EMB_D = (4, 260, 768)
EMB_PADS = ("none", "3", "absent")       # no padding id / id 3 / id V - 1, which the ids never hold
EMB_PATTERNS = ("random", "equal", "oob")  # oob: random with -1, V and V + 5 mixed in


class EmbCase(NamedTuple):
    id: str
    T: int
    V: int
    D: int
    pad_kind: str
    pattern: str

    @property
    def pad(self):
        return {"none": None, "3": 3, "absent": self.V - 1}[self.pad_kind]


def _em(T, V, D, pad_kind, pattern):
    return EmbCase(f"T{T}-V{V}-D{D}-pad_{pad_kind}-{pattern}", T, V, D, pad_kind, pattern)


def emb_cases():
    return [
        _em(0, 5, 4, "none", "random"),
        _em(1, 1, 4, "none", "random"),
        _em(63, 5, 260, "3", "random"),
        _em(64, 97, 4, "none", "equal"),
        _em(65, 1, 260, "none", "equal"),
        _em(65, 97, 768, "none", "oob"),
        _em(300, 97, 768, "3", "equal"),
        _em(300, 5, 4, "absent", "oob"),
        _em(8191, 97, 4, "3", "random"),
        _em(8192, 97, 260, "absent", "random"),
        _em(8193, 97, 4, "none", "oob"),
        _em(8193, 5, 768, "3", "random"),
    ]


def emb_ids(case, salt=0):
    """[T] int64 ids of the case (salt: another draw of the same pattern, for the second call)"""
    T, V = case.T, case.V
    g = torch.Generator().manual_seed(1000 * T + 10 * V + salt)
    hi = V - 1 if case.pad_kind == "absent" else V     # "absent": the padding id V - 1 never occurs
    if case.pattern == "equal":
        return torch.full((T,), (V // 2 + salt) % max(hi, 1), dtype=torch.int64)
    ids = torch.randint(0, max(hi, 1), (T,), generator=g)
    if case.pattern == "oob":
        bad = torch.tensor([-1, V, V + 5])
        where = torch.randperm(T, generator=g)[: max(3, T // 10)]
        ids[where] = bad[torch.arange(where.numel()) % 3]
    return ids
