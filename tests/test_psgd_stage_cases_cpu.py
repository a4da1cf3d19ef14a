"""tests/psgd_stage_cases.py reaches every PowerSGD P / Q / update kernel instance and every path
of csrc/powersgd.hip that depends on the plan: the coverage is asserted from the literals each case
claims, so that a bullet fails when it loses its last case, and (with the extension built) build_plan
reports the same facts under the case's NDP_PSGD_PKW.  Host code only."""
import collections

import pytest

from network_distributed_pytorch_amd.ops import native_available
from tests import psgd_stage_cases as C

N_CASES = 16
N_RUNS = {"p": 56, "q": 18, "u": 43}  # stage runs per input arm


def _mats(stage=None, pred=lambda c: True):
    """(case, i, n, m, r) of every matrix of the cases that run ``stage``"""
    for c in C.CASES:
        if stage is not None and not getattr(c, stage + "_vars"):
            continue
        if not pred(c):
            continue
        for i, ((n, m), r) in enumerate(zip(c.shapes, c.ranks)):
            yield c, i, n, m, r


def _q_offs(c):
    out, q = [], 0
    for (n, m), r in zip(c.shapes, c.ranks):
        out.append(q)
        q += m * r
    return out


def _rq(c):
    return 4 if c.max_rank <= 4 else 8 if c.max_rank <= 8 else 16


def test_case_list_is_well_formed():
    assert len(C.CASES) == N_CASES and len({c.name for c in C.CASES}) == N_CASES
    runs = collections.Counter(s for s, _, _ in C.stage_runs())
    assert runs == N_RUNS
    for c in C.CASES:
        k = len(c.shapes)
        assert all(len(t) == k for t in (c.offs, c.p_chunks, c.q_chunks, c.q_rows, c.compact_cols)), c.name
        assert c.supports is None or len(c.supports) == k
        assert all(n * m <= C.MAX_ELEMS for n, m in c.shapes), c.name
        assert c.kernels == C.instances(c.max_rank, c.p_cols), c.name
        # the claimed facts agree with each other
        for (n, m), pc, qc, rc in zip(c.shapes, c.p_chunks, c.q_chunks, c.q_rows):
            assert (pc - 1) * c.p_cols < m <= pc * c.p_cols, c.name
            assert (qc - 1) * rc < n <= qc * rc and rc <= 256, c.name
        for fuse, fused in c.p_vars:
            assert fuse in ("off", "on", "prev") and (c.wide or (not fused and fuse != "prev")), c.name
        assert c.wide or c.q_vars == (False,)
        for mode, lazy, hyper, q_div, r1 in c.u_vars:
            assert mode in (0, 1, 2, 3) and hyper in ("none", "wd0", "wd") and q_div in (1, 4)
            assert not lazy or (mode in (1, 2) and c.wide)
            assert mode != 3 or c.wide
            assert r1 == 0 or mode in (1, 2)
            if c.supports is not None:  # the compact tile: engine modes, no decay
                assert mode != 0 and hyper != "wd", c.name


def test_every_instance_has_a_case():
    P = {c.kernels[0] for c in C.CASES if c.p_vars}
    Q = {c.kernels[1] for c in C.CASES if c.q_vars}
    U = {c.kernels[2] for c in C.CASES if c.u_vars}
    assert P == {f"p_wide<{rq},{w}>" for rq in (4, 8, 16) for w in (256, 512, 1024)} | {"p<2>", "p<4>"}
    assert Q == {"q<1>", "q<2>", "q<4>"}
    assert U == {"update_wide<4>", "update_wide<8>", "update_wide<16>", "update"}
    # widths other than the rank's default come from NDP_PSGD_PKW
    for c in C.CASES:
        if c.wide:
            dflt = 512 if c.max_rank <= 8 else 1024
            assert (c.pkw is None) == (c.p_cols == dflt), c.name
    # ranks 17-32 and 33-64 for the narrow P
    assert {c.kernels[0]: c.max_rank for c in C.CASES if not c.wide} == {"p<2>": 24, "p<4>": 40}
    assert C.RANK1_SIZES == (1, 300, C.R1_STRIDE + 300)


def test_p_coverage():
    wide_fused = [c for c in C.CASES if c.wide and any(f for _, f in c.p_vars)]
    for rq in (4, 8, 16):  # the chunk classes at every RQ, summed by the launch's last arriver
        chunks = {pc for c in wide_fused if _rq(c) == rq for pc in c.p_chunks}
        assert 1 in chunks and any(2 <= k <= 8 for k in chunks) and 9 in chunks
        assert any(k >= 10 and 1 <= C.chunk_sum_tail(k)[1] <= 7 and C.chunk_sum_tail(k)[0] >= 1 for k in chunks)
        assert any(k >= 17 and C.chunk_sum_tail(k)[0] >= 2 for k in chunks)
    for c in C.CASES:
        if c.wide and c.supports is None and len(c.p_vars) == 4:  # every wide instance: all four variants
            assert set(c.p_vars) == {("off", True), ("on", True), ("prev", True), ("on", False)}
    assert {c.kernels[0] for c in C.CASES if set(c.p_vars) >= set(C.P_ALL)} >= {
        f"p_wide<{rq},{w}>" for rq in (4, 8, 16) for w in (256, 512, 1024)}
    assert {v for c in C.CASES if not c.wide for v in c.p_vars} == {("off", False), ("on", False)}

    mats = list(_mats("p"))
    wide = [(c, i, n, m, r) for c, i, n, m, r in mats if c.wide]
    assert any(n % 16 and n > 16 for _, _, n, _, _ in wide) and any(n % 4 and n > 4 for _, _, n, _, _ in wide)
    assert any(n < 4 for _, _, n, _, _ in wide)
    for group in (wide, [x for x in mats if not x[0].wide]):
        assert any(m % 4 != 0 for _, _, _, m, _ in group)
        assert any(m % 4 == 0 and c.offs[i] == 1 for c, i, _, m, _ in group)
        assert any(m % 4 == 0 and c.offs[i] == 0 for c, i, _, m, _ in group)
    for rq in (4, 8, 16):
        assert any(r < rq for c, _, _, _, r in wide if _rq(c) == rq)  # the clamp min(n, m, R)
    assert any(r % 4 for _, _, _, _, r in wide)
    for rq in (4, 8, 16):  # both Q load forms: float4 rows, and scalar at r % 4 == 0 behind an odd m r
        q4 = {(_q_offs(c)[i] % 4 == 0) for c, i, _, _, r in wide if _rq(c) == rq and r % 4 == 0}
        assert q4 == {True, False}, rq
        assert any(_q_offs(c)[i] % 4 and (c.shapes[i - 1][1] * c.ranks[i - 1]) % 2
                   for c, i, _, _, r in wide if _rq(c) == rq and r % 4 == 0 and i > 0)


def test_q_coverage():
    one_plan = [c for c in C.CASES if True in c.q_vars and 1 in c.q_chunks
                and any(2 <= k <= C.Q_FIN_MAX for k in c.q_chunks) and any(k > C.Q_FIN_MAX for k in c.q_chunks)]
    assert one_plan, "finished in-kernel and left to seg_reduce in one launch"
    assert any(False in c.q_vars for c in one_plan)  # and the unfused finish of the same plan
    for ncg in (1, 2, 4):
        cs = [c for c in C.CASES if c.q_vars and c.kernels[1] == f"q<{ncg}>"]
        rows = {rc for c in cs for rc in c.q_rows}
        assert {64, 68, 100, 256} <= rows, ncg
        last = {n - (qc - 1) * rc for c in cs for (n, _), qc, rc in zip(c.shapes, c.q_chunks, c.q_rows) if qc > 1}
        assert {1, 17} <= last and any(n % rc == 0 and qc > 1 for c in cs
                                       for (n, _), qc, rc in zip(c.shapes, c.q_chunks, c.q_rows)), ncg
        assert {m for c in cs for _, m in c.shapes} >= ({5, 300, 1030} if ncg == 1 else {300, 1030}), ncg
        assert any(False in c.q_vars for c in cs), ncg
    # the third and later batches of the double-buffered loop: more than 64 rows per item
    assert any(rc > 64 for c in C.CASES if c.q_vars for rc in c.q_rows)


def test_update_coverage():
    wide = [v for c in C.CASES if c.wide for v in c.u_vars]
    narrow = [v for c in C.CASES if not c.wide for v in c.u_vars]
    assert {v[0] for v in wide} == {0, 1, 2, 3} and {v[0] for v in narrow} == {0, 1, 2}
    for mode in (1, 2):
        assert {v[1] for v in wide if v[0] == mode} == {True, False}
    for vs in (wide, narrow):
        assert {v[2] for v in vs} == {"none", "wd0", "wd"}
        assert {v[3] for v in vs} == {1, 4}
    for rq in (4, 8, 16):
        vs = [v for c in C.CASES if c.u_vars and c.kernels[2] == f"update_wide<{rq}>" for v in c.u_vars]
        assert {1, 300, C.R1_STRIDE + 300} <= {v[4] for v in vs}, rq  # the rank-1 tail in the launch
        assert {v[0] for v in vs} == {0, 1, 2, 3} and {v[1] for v in vs} == {True, False}
    assert any(v[4] for v in narrow)
    mats = list(_mats("u"))
    for tiles, group in (((16, 256), [x for x in mats if x[0].wide]), ((64, 64), [x for x in mats if not x[0].wide])):
        assert any(n % tiles[0] and n > tiles[0] for _, _, n, _, _ in group)
        assert any(m % tiles[1] and m > tiles[1] for _, _, _, m, _ in group)
        assert any(m % 4 for _, _, _, m, _ in group) and any(m % 4 == 0 and c.offs[i] for c, i, _, m, _ in group)
        assert any(m % 4 == 0 and not c.offs[i] for c, i, _, m, _ in group)


def test_dead_tap_coverage():
    tapped = [c for c in C.CASES if c.supports is not None]
    assert {_rq(c) for c in tapped} == {4, 8, 16}
    assert any(_rq(c) == 4 for c in tapped) and any(_rq(c) in (8, 16) and c.p_cols == 1024 for c in tapped)
    want = {(4, 1), (9, 1), (9, 4), (9, 6), (16, 9), (16, 15)}
    for c in tapped:
        got = {(T, bin(mask).count("1")) for i, (T, mask) in enumerate(c.supports) if c.support(i)}
        assert got == want, c.name
        assert (9, 1 << 4) in c.supports and (9, 0b110110000) in c.supports
        for i, (T, mask) in enumerate(c.supports):
            if c.support(i):
                L = bin(mask).count("1")
                assert c.compact_cols[i] == c.shapes[i][1] // T * L
            else:
                assert c.compact_cols[i] == c.shapes[i][1]
        assert any(c.support(i) is None for i in range(len(c.shapes)))  # a full matrix in the same launches
        assert any(cc % 4 for i, cc in enumerate(c.compact_cols) if c.support(i))
        assert any(cc % 4 == 0 for i, cc in enumerate(c.compact_cols) if c.support(i))
        assert any(cc > 256 for i, cc in enumerate(c.compact_cols) if c.support(i))  # several column blocks
        assert any(qc > 1 for i, qc in enumerate(c.q_chunks) if c.support(i))
        assert any(qc > C.Q_FIN_MAX for i, qc in enumerate(c.q_chunks) if c.support(i))
        assert any(pc > 1 for i, pc in enumerate(c.p_chunks) if c.support(i))
        # all three stages, lazy and eager, and mode 3
        assert {f for f, _ in c.p_vars} == {"off", "on", "prev"} and {f for _, f in c.p_vars} == {True, False}
        assert set(c.q_vars) == {True, False}
        assert {v[0] for v in c.u_vars} == {1, 2, 3} and {v[1] for v in c.u_vars} == {True, False}


@pytest.mark.skipif(not native_available(), reason="extension not built")
def test_build_plan_reports_each_case(monkeypatch):
    from network_distributed_pytorch_amd.ops import ext

    X = ext()
    for c in C.CASES:
        if c.pkw is None:
            monkeypatch.delenv("NDP_PSGD_PKW", raising=False)
        else:
            monkeypatch.setenv("NDP_PSGD_PKW", str(c.pkw))
        d = X.build_plan([tuple(s) for s in c.shapes], c.rank, [tuple(s) for s in c.supports] if c.supports else [])
        got = (int(d["p_cols"]), tuple(d["p_chunks"]), tuple(d["q_chunks"]), tuple(d["q_rows"]),
               tuple(d["compact_cols"]), C.instances(int(d["max_rank"]), int(d["p_cols"])), tuple(d["ranks"]))
        want = (c.p_cols, c.p_chunks, c.q_chunks, c.q_rows, c.compact_cols, c.kernels, c.ranks)
        assert got == want, c.name
