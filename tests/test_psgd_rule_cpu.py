"""The stage oracle of tests/psgd_rule.py checked against itself: the stages compose to the round
oracle, lazy error feedback equals eager on the int arm, the op-by-op chain equals a numpy.float32
chain bitwise on the mantissa arm, the int arm stays exact for every case, and the dead-tap maps are
the MatGeom ones.  No extension, no GPU."""
import numpy as np
import torch

from tests import oracle
from tests import psgd_rule as R
from tests import psgd_stage_cases as C


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_stages_compose_to_the_round_oracle():
    gen = _gen(1)
    for n, m, r in ((40, 70, 4), (9, 130, 8), (64, 33, 16)):
        M = torch.randn(n, m, generator=gen)
        Q = torch.randn(m, r, generator=gen)
        outs, mems, newq = oracle.powersgd_round([[M]], [Q], r)
        P, kept = R.p_stage(M, Q)
        assert kept is None
        P_hat = oracle.mgs(P)
        Qn = R.q_stage(M, P_hat)
        assert torch.equal(Qn, newq[0])  # the same fp64 products: no rounding before the update stage
        u = R.update_stage(0, P_hat, Qn, 1.0, M=M)
        # the update stage rounds Qs, out and mem to fp32 once each
        tol = 4 * R.EPS32 * float(outs[0].abs().max() + M.abs().max())
        assert (u["out"] - outs[0]).abs().max() <= tol
        assert (u["mem"] - mems[0][0]).abs().max() <= tol
        assert (u["q_warm"] - newq[0]).abs().max() <= R.EPS32 * float(newq[0].abs().max())


def test_lazy_equals_eager_on_the_int_arm():
    gen = _gen(2)
    for n, m, r, q_div in ((18, 300, 4, 1), (5, 67, 5, 4), (33, 1030, 16, 4)):
        g1, e0, g2 = (R.stream("int", gen, (n, m)) for _ in range(3))
        Q0 = R.small_q("int", gen, m, r, 256)
        P_hat = R.small_p_rows("int", gen, n, r)
        Q_sum = R.stream("int", gen, (m, r), 2) * q_div
        mom, x = R.stream("int", gen, (n, m)), R.stream("int", gen, (n, m))
        _, M1 = R.p_stage(g1, Q0, e=e0)
        kw = dict(mom=mom, x=x, lr=R.LR, momentum=R.MOMENTUM, wd=R.WD)
        eager = R.update_stage(1, P_hat, Q_sum, q_div, M=M1.float(), **kw)
        lazy = R.update_stage(1, P_hat, Q_sum, q_div, lazy=True, **kw)
        assert "e" not in lazy and torch.equal(lazy["p_prev"], P_hat.double())
        for k in ("q_warm", "mom", "x"):
            assert torch.equal(eager[k], lazy[k])
        Qs = eager["q_warm"].float()
        Pe, Me = R.p_stage(g2, Qs, e=eager["e"].float())
        Pl, Ml = R.p_stage(g2, Qs, e=M1.float(), p_prev=lazy["p_prev"].float())
        assert torch.equal(Pe, Pl) and torch.equal(Me, Ml)
        assert torch.equal(Pe.float().double(), Pe)  # exact in fp32


def test_rule_equals_numpy_float32_chain_on_the_mantissa_arm():
    gen = _gen(3)
    n, m, r = 400, 500, 4  # 200k elements
    f32 = np.float32
    for q_div, wd in ((1.0, 0.0), (4.0, R.WD)):
        P_hat = R.small_p_rows("mantissa", gen, n, r)
        Q_sum = R.stream("mantissa", gen, (m, r))
        M, mom, x = (R.stream("mantissa", gen, (n, m)) for _ in range(3))
        got = R.update_stage(2, P_hat, Q_sum, q_div, M=M, mom=mom, x=x, lr=R.LR, momentum=R.MOMENTUM, wd=wd)
        # numpy.float32, op by op; the one nonzero of a P-hat row makes out a single exact product, and
        # wd x and lr up are exact (powers of two), so a * b + c in two fp32 ops is the fused op
        Qs = (Q_sum.numpy() / f32(q_div)).astype(f32)
        col = P_hat.abs().argmax(1).numpy()
        pv = P_hat.numpy()[np.arange(n), col]
        out = (pv[:, None] * Qs[:, col].T).astype(f32)
        assert out.dtype == f32
        e = M.numpy() - out
        d = (f32(wd) * x.numpy() + out) if wd != 0 else out
        mm = mom.numpy() * f32(R.MOMENTUM) + d
        up = d + mm
        xx = x.numpy() - f32(R.LR) * up
        for k, v in (("q_warm", Qs), ("e", e), ("mom", mm), ("g", up), ("x", xx)):
            assert v.dtype == f32
            assert torch.equal(got[k], torch.from_numpy(v).double()), k
        # and the absolute twin bounds it
        S = R.update_stage(2, P_hat, Q_sum, q_div, M=M, mom=mom, x=x, lr=R.LR, momentum=R.MOMENTUM, wd=wd,
                           absolute=True)
        for k in got:
            assert (got[k].abs() <= S[k] * (1 + 8 * R.EPS32)).all(), k


def test_mantissa_selectors_sit_at_the_edges():
    gen = _gen(4)
    for length, count, chunk in ((9228, 16, 1024), (300, 4, 512), (7, 3, 256), (2113, 12, 64), (5, 5, 256)):
        pos = R.selector_positions(gen, length, count, chunk)
        assert len(set(pos)) == count and 0 in pos and length - 1 in pos
        tail0 = (length - 1) // chunk * chunk
        assert count < 3 or any(tail0 <= p < length for p in pos)
        Q = R.small_q("mantissa", gen, length, count, chunk)
        assert ((Q != 0).sum(0) == 1).all() and ((Q != 0).sum(1) <= 1).all()
        assert torch.equal(torch.log2(Q[Q != 0].abs()).round(), torch.log2(Q[Q != 0].abs()))
    P = R.small_p_rows("mantissa", gen, 33, 8)
    assert ((P != 0).sum(1) == 1).all() and P[0, 0] != 0 and P[32, 7] != 0
    v = R.stream("mantissa", gen, (4096,))
    assert (v.abs() >= 2.0 ** -4).all() and (v.abs() < 2.0 ** 5).all()
    mant = (v.abs().double() / torch.pow(2.0, torch.floor(torch.log2(v.abs().double())))) * (1 << 23)
    assert torch.equal(mant, mant.round()) and (mant % 2 == 1).float().mean() > 0.4  # the last bit is used


def test_int_arm_stays_exact_for_every_case():
    for c in C.CASES:
        for (n, m), r in zip(c.shapes, c.ranks):
            for stage in ("p", "q", "u"):
                assert R.int_bound(stage, n, m, r) < 2 ** 24, (c.name, n, m, stage)
    assert R.int_bound("p", 9300, 9300, 16) == 9300 * 70 * 2 and R.int_bound("q", 16400, 6, 6) < 2.3e6
    # the bound is reached by the rule at the limits, and the rule is exact there
    n, m, r = 3, 18436, 3
    g, e = torch.full((n, m), 3.0), torch.full((n, m), 3.0)
    Q, pp = torch.full((m, r), 2.0), torch.full((n, r), -2.0)
    P, M = R.p_stage(g, Q, e=e, p_prev=pp)
    assert float(M.max()) == 3 + 3 + r * 4 and float(P.max()) == m * (6 + 4 * r) * 2 <= R.int_bound("p", n, m, r)
    assert torch.equal(P.float().double(), P)


def test_dead_tap_maps_follow_matgeom():
    # compact column j is full column (j // L) * T + tap[j % L], taps ascending
    assert R.live_taps(9, 0b110110000) == [4, 5, 7, 8]
    assert R.full_columns(18, 9, 1 << 4).tolist() == [4, 13]
    assert R.full_columns(18, 9, 0b110110000).tolist() == [4, 5, 7, 8, 13, 14, 16, 17]
    assert R.full_columns(32, 16, 0x0FF8).tolist() == list(range(3, 12)) + list(range(19, 28))
    for c in C.CASES:
        for i, (n, m) in enumerate(c.shapes):
            s = c.support(i)
            if s is None:
                continue
            full = torch.arange(n * m, dtype=torch.float32).view(n, m)
            comp = R.compress(full, *s)
            assert comp.shape == (n, c.compact_cols[i])
            back = R.expand(comp, m, *s, fill=-1.0)
            live = back >= 0
            assert torch.equal(back[live], full[live]) and int(live.sum()) == comp.numel()
            assert live[0].tolist() == [bool(s[1] >> (j % s[0]) & 1) for j in range(m)]
