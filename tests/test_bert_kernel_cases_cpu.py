"""tests/bert_kernel_cases.py leaves no DistilBERT kernel instance or launch geometry out, and
tests/bert_rule.py's twins give the geometry each class claims.  No GPU, no extension."""
import os
import re

import pytest
import torch

from network_distributed_pytorch_amd.ops.attention import dropout_keep_mask
from network_distributed_pytorch_amd.ops.layernorm import ln_keep_mask
from tests import bert_kernel_cases as C
from tests import bert_rule as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "network_distributed_pytorch_amd",
                    "csrc")
LN, ATTN, COL, EMB = C.ln_cases(), C.attn_cases(), C.col_cases(), C.emb_cases()


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_case_ids_are_unique_and_none_is_missing():
    for cases in (LN, ATTN, COL, EMB):
        ids = [c.id for c in cases]
        assert len(set(ids)) == len(ids)
    # 4 D x 3 modes x 2 x 4 row classes + 12 + 3 deferred + the negative seed + 2 gap cases; 5 N x 6 M + 3 + 1
    assert (len(LN), len(ATTN), len(COL), len(EMB)) == (96 + 15 + 1 + 2, 21, 30 + 3 + 1, 12)


# ------------------------------------------------ LayerNorm ------------------------------------------------
def _ln_switch_arms():
    """the <V, DM> arms of LN_SWITCH, read from the source"""
    src = _src("layernorm.hip")
    body = src[src.index("#define LN_SWITCH"):src.index("template <int V, int DM>\nstatic void ln_fwd_go")]
    return [(int(v), int(dm)) for v, dm in re.findall(r"K<\s*(\d+)\s*,\s*(\d+)\s*>", body)]


def test_every_ln_switch_arm_has_a_case():
    arms = _ln_switch_arms()
    assert len(arms) == 12 and len(set(arms)) == 12, arms
    assert set(arms) == {(D // 256, m) for D in C.LN_D for m in C.LN_MODES}
    # launch_ln_fwd and launch_ln_bwd both go through the switch: a case runs both kernels
    src = _src("layernorm.hip")
    assert len(re.findall(r"^\s*LN_SWITCH\(", src, re.M)) == 2
    assert {c.instance for c in LN} == set(arms)


def test_ln_row_classes_for_every_instance():
    have = {(c.D, c.mode, c.res, c.R) for c in LN if not c.deferred}
    for D in C.LN_D:
        for m in C.LN_MODES:
            for res in (False, True):
                for Rr in C.LN_ROWS:
                    assert (D, m, res, Rr) in have, (D, m, res, Rr)
            assert any(c.deferred and (c.D, c.mode) == (D, m) and R.ln_bwd_wgs(c.R) > 1 for c in LN), (D, m)
    assert any(c.deferred and R.ln_bwd_wgs(c.R) == 1 for c in LN)       # a single slab
    assert any(c.seed < 0 and c.mode for c in LN)
    assert {c.mode for c in LN if c.gap} == {1, 2}
    assert all(c.p == 0.1 for c in LN)


def test_ln_geometry_twins():
    assert [R.ln_bwd_wgs(r) for r in (1, 3, 4, 5, 9, 2048, 2049, 2051)] == [1, 1, 1, 2, 3, 512, 512, 512]
    assert [R.rows_per_wave(r) for r in (1, 3, 9, 2048, 2049, 2051)] == [1, 1, 1, 1, 2, 2]
    # R = 2051: 2048 wave slots of 2 rows; slot 1025 holds row 2050 alone, the slots after it are idle
    rpw = R.rows_per_wave(2051)
    held = [max(0, min(2051, (w + 1) * rpw) - w * rpw) for w in range(4 * R.ln_bwd_wgs(2051))]
    assert held[:1025] == [2] * 1025 and held[1025] == 1 and not any(held[1026:])
    # R = 9: three workgroups, the last with one row; R = 3: a partial workgroup
    assert R.ln_bwd_wgs(9) == 3 and R.ln_bwd_wgs(3) == 1


def test_ln_gap_cases():
    g = C.LN_GAP
    lo, hi = R.thr64(g["p"]), R.thr32(g["p"])
    assert lo < hi
    assert lo <= int(R.ln_hash(g["seed"], g["row"], g["col"])) < hi
    assert C.search_ln_gap(g["p"], g["R"], g["D"], start=g["seed"] - 1) == (g["seed"], (g["row"], g["col"]))
    assert bool(ln_keep_mask(g["seed"], g["R"], g["D"], g["p"])[g["row"], g["col"]])   # the twin keeps it
    for c in LN:
        if c.gap:
            assert (c.p, c.R, c.D, c.seed, c.gap) == (g["p"], g["R"], g["D"], g["seed"], (g["row"], g["col"]))


# ------------------------------------------------ attention ------------------------------------------------
def test_attention_classes_present():
    assert {c.S for c in ATTN} >= set(C.ATTN_S) | {C.LONG_S}
    assert {c.H for c in ATTN} == set(C.ATTN_H) | {2}
    for S in C.ATTN_S:
        assert {c.H for c in ATTN if c.S == S} >= set(C.ATTN_H), S
    assert {c.pattern for c in ATTN} == set(C.ATTN_PATTERNS)
    assert {c.p > 0 for c in ATTN if c.pattern == "padded"} == {False, True}
    assert {c.packed for c in ATTN} == {False, True}
    assert {(c.packed, c.p > 0) for c in ATTN} == {(a, b) for a in (False, True) for b in (False, True)}
    assert any(c.seed < 0 and c.p > 0 for c in ATTN)
    assert {c.S for c in ATTN if c.pattern == "first"} == {129, 200}
    assert {c.S for c in ATTN if c.pattern == "middle"} == {200}
    long = [c for c in ATTN if c.pattern == "long"]
    assert [(c.B, c.S, c.H, c.p) for c in long] == [(1, C.LONG_S, 1, 0.0)]


def _blocks(row):
    """per 64-key block: 'dead' (no attended key), 'live' (all attended) or 'mixed'"""
    out = []
    for k0 in range(0, len(row), 64):
        b = row[k0:k0 + 64]
        out.append("dead" if not any(b) else ("live" if all(b) else "mixed"))
    return out


def test_attention_masks_are_what_they_claim():
    kmax = int(re.search(r"constexpr int kMaxBlk = (\d+);", _src("attention.hip")).group(1))
    for c in ATTN:
        m = C.attn_mask(c)
        if c.pattern == "none":
            assert m is None
            continue
        assert len(m) == c.B and all(len(r) == c.S for r in m)
        b0 = _blocks(m[0])
        if c.pattern in ("tail", "padded"):
            start = m[0].index(0)
            assert 0 < start and start % 64 and not any(m[0][start:]) and all(m[0][:start]), c.id
        if c.pattern == "padded":
            assert not any(m[1]) and len(_blocks(m[1])) > 1 and any(m[0])
        else:
            assert all(any(r) for r in m), c.id          # no other pattern pads a whole row
        if c.pattern == "first":
            assert b0[0] == "dead" and "dead" not in b0[1:]
        if c.pattern == "middle":
            assert b0 == ["live", "dead", "live", "live"]
        if c.pattern == "long":
            assert len(b0) == kmax + 1                   # block kMaxBlk exists: outside the map
            assert b0[2] == "dead" and b0[kmax] == "mixed" and b0.count("dead") == 1


def test_attention_gap_cases():
    gaps = [c for c in ATTN if c.gap]
    assert sorted(c.p for c in gaps) == [0.1, 0.2, 0.3]
    for c in gaps:
        assert (c.B * c.H, c.S, c.pattern) == (2, C.GAP_S, "none")
        lo, hi = R.thr64(c.p), R.thr32(c.p)
        assert lo < hi
        bh, q, k = c.gap
        assert lo <= int(R.attn_hash(c.seed, bh, q, k)) < hi, c.id
        assert C.search_attn_gap(c.p, 2, C.GAP_S, start=c.seed - 1) == (c.seed, c.gap), c.id
        keep = dropout_keep_mask(c.seed, c.B, c.H, c.S, c.p).view(c.B * c.H, c.S, c.S)
        assert bool(keep[bh, q, k]), c.id                # the twin (double threshold) keeps it
    assert (R.thr64(0.1), R.thr32(0.1)) == (429496729, 429496736)
    assert (R.thr64(0.3), R.thr32(0.3)) == (1288490188, 1288490240)
    assert R.thr32(0.2) - R.thr64(0.2) == 13
    assert int(R.attn_hash(55741, 0, 53, 51)) == 429496731 and int(R.attn_hash(1811, 0, 1, 29)) == 1288490217


@pytest.mark.parametrize("seed", [0, 7, 12345, -12345, 2 ** 31 - 1, -2 ** 31])
def test_ops_twins_equal_the_rule_hashes(seed):
    for p in (0.1, 0.3, 0.999999):
        a = dropout_keep_mask(seed, 2, 3, 70, p).view(6, 70, 70)
        assert torch.equal(a, R.attn_keep(seed, 6, 70, p))
        assert torch.equal(ln_keep_mask(seed, 37, 1024, p), R.ln_keep(seed, 37, 1024, p))
    assert R.thr64(1.0 - 2.0 ** -40) == 0xFFFFFFFF and R.thr64(0.5) == 2 ** 31


# ---------------------------------------- column sums, GELU backward ---------------------------------------
def test_colsum_classes_present():
    have = {(c.M, c.N) for c in COL}
    assert have >= {(M, N) for N in C.COL_N for M in C.COL_M}
    assert C.CAP_MN in have and R.colsum_chunks(*C.CAP_MN) == 1024
    assert R.colsum_chunks(C.CAP_MN[0] * 2, C.CAP_MN[1]) == 1024     # the cap, not the 32-row floor
    assert R.colsum_chunks(C.CAP_MN[0] - 32, C.CAP_MN[1]) == 1023
    for n in C.COL_GROUP_ROWS:
        M = C.boundary_m(n)
        assert (M, C.BOUNDARY_N) in have and R.group_rows(M, C.BOUNDARY_N) == [[n] * 4]
    assert [C.boundary_m(n) for n in C.COL_GROUP_ROWS] == [12, 16, 20]
    unroll = int(re.search(r"constexpr int kColUnroll = (\d+);", _src("linear.hip")).group(1))
    assert C.COL_GROUP_ROWS == (unroll - 1, unroll, unroll + 1)


def test_colsum_geometry_twins():
    assert [R.colsum_strips(N) for N in C.COL_N] == [1, 1, 1, 2, 3]
    assert 260 // 4 - 64 == 1                                        # the second strip has one live lane
    assert [R.colsum_chunks(M, 768) for M in C.COL_M] == [1, 1, 1, 1, 2, 4]
    assert R.rows_per_chunk(33, 768) == 17 and R.rows_per_chunk(100, 768) == 25
    assert R.group_rows(33, 768) == [[5, 4, 4, 4], [4, 4, 4, 4]]
    assert R.group_rows(1, 4) == [[1, 0, 0, 0]] and R.group_rows(5, 4) == [[2, 1, 1, 1]]
    assert R.colsum_chunks(8192, 3072) == 86 and R.colsum_chunks(8192, 768) == 256
    assert len(C.GELU_SPECIALS) == 12 and {abs(x) for x in C.GELU_SPECIALS} == {0.0, 1e-30, 0.5, 3.0, 10.0, 40.0}


# ------------------------------------------------ embedding ------------------------------------------------
def test_embedding_classes_present():
    assert {c.T for c in EMB} == set(C.EMB_T)
    assert {c.V for c in EMB} == set(C.EMB_V)
    assert {c.D for c in EMB} == set(C.EMB_D)
    assert {c.pad_kind for c in EMB} == set(C.EMB_PADS)
    assert {c.pattern for c in EMB} == set(C.EMB_PATTERNS)
    src = _src("embedding.hip")
    tile = int(re.search(r"constexpr int kEmbTile = (\d+);", src).group(1))
    assert {tile - 1, tile, tile + 1, 63, 64, 65, 0} <= set(C.EMB_T)
    for c in EMB:
        assert c.pattern != "equal" or c.T <= 300
        assert c.pad is None or 0 <= c.pad < c.V, c.id
        for salt in (0, 1):
            ids = C.emb_ids(c, salt)
            assert ids.shape == (c.T,) and ids.dtype == torch.int64
            if c.pad_kind == "absent":
                assert not (ids == c.pad).any(), c.id
            if c.pattern == "equal":
                assert (ids == ids[0]).all() and ids[0] != c.pad and 0 <= ids[0] < c.V
            if c.pattern == "oob":
                assert {-1, c.V, c.V + 5} <= set(ids.tolist()), c.id
            else:
                assert ((ids >= 0) & (ids < c.V)).all()
        if c.V > 2 and c.T > 1 and c.pattern != "equal":
            assert not torch.equal(C.emb_ids(c, 0), C.emb_ids(c, 1))


# ------------------------------------------- the order emulations ------------------------------------------
def test_order_emulations_agree_with_fp64_and_exact_integers():
    """integer data sums exactly in any order: every emulation must give the plain sum bitwise"""
    g = torch.Generator().manual_seed(0)
    for M, N in ((1, 4), (33, 260), (100, 768), (2051, 8)):
        x = torch.randint(-8, 9, (M, N), generator=g).float()
        assert torch.equal(R.colsum_order(x), x.sum(0))
        assert R.colsum_partials_order(x).shape == (R.colsum_chunks(M, N), N)
        assert torch.equal(R.ln_dbeta_order(x), x.sum(0))
        assert R.ln_dbeta_partials_order(x).shape == (R.ln_bwd_wgs(M), N)
    ids = torch.tensor([3, 1, -1, 3, 7, 2, 3, 5, 9, 1])
    go = torch.randint(-8, 9, (10, 4), generator=g).float()
    got = R.embedding_bwd_order(ids, go, 5, 2)
    assert torch.equal(got.double(), R.embedding_bwd_rule(ids, go, 5, 2))
    assert torch.equal(got[3], go[0] + go[3] + go[6]) and not got[[0, 2, 4]].any()
    part = torch.randint(-8, 9, (37, 12), generator=g).float()
    assert torch.equal(R.slab_sum_order(part, 37, 12), part.sum(0))
