"""``psgd_update_adam`` / ``rank1_adam_step`` (csrc/powersgd.hip) on their own, the way
tests/test_psgd_stages_gpu.py drives ``psgd_update``: sentinel-filled arenas, every written buffer
compared whole (guard bands included), every input that must not be written compared too, every launch
run twice from the same state (the second run also proves that the tickets were re-armed).

What is compared with what:
  o (the decompressed value, read from a mode-2 launch on the same inputs) against psgd_rule.update_stage's
    ``out``: bitwise on the int and mantissa arms, within (K + 8) 2^-24 S on Gaussians, K = r + 1 (the quotient
    and r fmaf), S the rule on absolute values;
  m', v', x' against tests/adamw_rule.py applied to the device's own o: bitwise on all three arms (the chain
    is single correctly rounded operations); e against fl(M - o) likewise, and against update_stage on the
    exact arms; p_prev and q_warm against update_stage, bitwise.
"""
import numpy as np
import pytest
import torch

from network_distributed_pytorch_amd.ops import StateBlock, ext
from network_distributed_pytorch_amd.parallel.powersgd import _PlanBuffers
from tests import adamw_rule as A
from tests import psgd_rule as R
from tests import psgd_stage_cases as C
from tests.test_psgd_stages_gpu import GUARD, SENT, Arena, _bind, _flat, _gen, _plan

pytestmark = pytest.mark.gpu

F = np.float32
PLANS = ("wide-r4-pkw512-default", "wide-r8-pkw512-default", "wide-r16-pkw1024-default", "tall-r4")
LR, WD, BETAS, EPS = 0.01, 0.125, (0.9, 0.99), 1e-8
BLOCK0 = (0.729, 0.9703, 3)  # the block before the launch: not the initial one
# (mode, lazy, q_div, r1 elements, wd, decay_1d)
VARIANTS = ((1, False, 4, 300, WD, True), (1, True, 1, 1, 0.0, False), (2, False, 4, C.R1_STRIDE + 300, WD, False),
            (2, True, 1, 0, 0.0, True))


def _i32(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(got, want, what):
    got, want = _i32(got), _i32(want.float())
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = int(bad[0])
        raise AssertionError(f"{what}: element {i} is {got.view(torch.float32)[i].item()!r}, expected "
                             f"{want.view(torch.float32)[i].item()!r} ({len(bad)} of {got.numel()} differ)")


def _roundup(n, k):
    return (n + k - 1) // k * k


class Setup:
    """one plan bound to sentinel-filled arenas, with the Adam state next to it"""

    def __init__(self, B, case_offs, arm, gen, q_div, r1n, device):
        self.B, self.device, self.q_div, self.r1n = B, device, q_div, r1n
        self.shapes, self.ranks = list(B.shapes), list(B.ranks)
        k = len(self.shapes)
        self.P, self.Qsum, ins = [], [], {nm: [] for nm in ("M", "mom", "v", "x", "g")}
        for (n, m), r in zip(self.shapes, self.ranks):
            self.P.append(R.small_p_rows(arm, gen, n, r))
            self.Qsum.append(R.stream(arm, gen, (m, r), 2) * (q_div if arm == "int" else 1))
            ins["M"].append(R.stream(arm, gen, (n, m)))
            ins["mom"].append(R.stream(arm, gen, (n, m)))
            ins["v"].append(R.stream(arm, gen, (n, m)).abs())
            ins["x"].append(R.stream(arm, gen, (n, m)))
            ins["g"].append(R.stream(arm, gen, (n, m)))
        self.ins = ins
        sz = [n * m for n, m in self.shapes]
        offs = list(case_offs)
        self.ar = Arena(sz, offs)                                       # M, x, g
        self.mv = Arena(sz + ([r1n] if r1n else []), offs + [1])        # m and v, the rank-1 slot 4 bytes off
        self.r1 = None
        if r1n:
            self.r1 = {nm: R.stream(arm, gen, (r1n,)) for nm in ("buf", "mom", "x")}
            self.r1["v"] = R.stream(arm, gen, (r1n,)).abs()
            self.ra = Arena([r1n], [1])
        self.v_delta = _roundup(self.mv.total, 4)
        mo = torch.full((2 * self.v_delta,), SENT)
        mo[: self.mv.total] = self.mv.fill(ins["mom"] + ([self.r1["mom"]] if r1n else []))
        mo[self.v_delta: self.v_delta + self.mv.total] = self.mv.fill(ins["v"] + ([self.r1["v"]] if r1n else []))
        self.host = {"M": self.ar.fill(ins["M"]), "x": self.ar.fill(ins["x"]), "g": self.ar.fill(ins["g"]), "mo": mo,
                     "pp": torch.full((B.p_total + 2 * GUARD,), SENT),
                     "comm": torch.cat([_flat(B.p_offs, B.p_total, self.P), torch.full((B.r1_numel,), SENT)]),
                     "qm": _flat(B.q_offs, B.q_total, self.Qsum)}
        if r1n:
            self.host["comm"][B.p_total: B.p_total + r1n] = self.r1["buf"]
            self.host["r1x"], self.host["r1g"] = self.ra.fill([self.r1["x"]]), self.ra.fill([None])
        self.dev = {nm: t.to(device) for nm, t in self.host.items()}
        rows = []
        for i in range(k):
            p = {nm: self.ar.ptr(self.dev[nm], i) for nm in ("M", "x", "g")}
            rows.append([p["g"], p["M"], p["M"], 0, 0, self.mv.ptr(self.dev["mo"], i), p["x"], p["g"]])
        _bind(B, rows)
        X = ext()
        self.block = StateBlock(device, ("b1pow", "b2pow", "steps"), BLOCK0)
        self.ctr = torch.zeros(X.arrive_ctr_words(B.counts["n_u_items"] + 1024), dtype=torch.int32, device=device)
        self.hyper = torch.zeros(4, device=device)

    def reset(self, lr=LR, wd=0.0, block=BLOCK0):
        B = self.B
        for nm, t in self.host.items():
            if nm not in ("comm", "qm"):
                self.dev[nm].copy_(t)
        B.comm_buf.copy_(self.host["comm"])
        B.q_memory.copy_(self.host["qm"])
        B.q_warm.fill_(SENT)
        self.hyper.copy_(torch.tensor([lr, wd, 0.0, 0.0]))
        if block is not None:
            self.block.write(dict(zip(("b1pow", "b2pow", "steps"), block)))

    def p_prev(self, lazy):
        return self.dev["pp"][GUARD: GUARD + self.B.p_total] if lazy else None

    def r1_args(self, write_g):
        if not self.r1n:
            return {}
        s = self.mv.starts[-1]
        sl = slice(self.ra.starts[0], self.ra.starts[0] + self.r1n)
        return dict(r1_buf=self.B.rank1_buf[: self.r1n], r1_div=float(self.q_div), r1_mom=self.dev["mo"][s: s + self.r1n],
                    r1_x=self.dev["r1x"][sl], r1_g=self.dev["r1g"][sl] if write_g else None)

    def launch(self, mode, lazy, decay_1d, advance=True, items=None, r1=True, **over):
        B = self.B
        kw = dict(geom_host=B._geom_host, hyper=self.hyper, block=self.block.dev, ctr=self.ctr, moments=self.dev["mo"],
                  v_delta=self.v_delta, beta1=BETAS[0], beta2=BETAS[1], eps=EPS, decay_1d=decay_1d, advance=advance,
                  p_prev=self.p_prev(lazy), max_rank=B.max_rank)
        kw.update(self.r1_args(mode == 2) if r1 else {})
        kw.update(over)
        max_rank = kw.pop("max_rank")
        ext().psgd_update_adam(B.geom, B.ptrs, B.u_items if items is None else items, B.comm_buf, B.q_memory,
                               float(self.q_div), B.q_warm, mode, max_rank, **kw)
        torch.cuda.synchronize()

    def snapshot(self):
        out = {nm: t.detach().cpu().clone() for nm, t in self.dev.items() if nm not in ("comm", "qm")}
        out.update(comm=self.B.comm_buf.cpu().clone(), qm=self.B.q_memory.cpu().clone(), qw=self.B.q_warm.cpu().clone(),
                   block=self.block.read(), ctr=self.ctr.cpu().clone())
        return out

    def o_of(self, snap):
        """the device's own decompressed values, from the g arena of a mode-2 snapshot"""
        return [snap["g"][s: s + n * m].view(n, m).clone() for s, (n, m) in zip(self.ar.starts, self.shapes)]


def _rule(x, o, mom, v, block, wd, div=1.0, decays=True):
    blk = (F(block[0]), F(block[1]), block[2])
    xo, mo, vo, nb = A.step_arrays(x.numpy(), o.numpy(), mom.numpy(), v.numpy(), blk, LR, wd, *BETAS, EPS, div, decays)
    return torch.from_numpy(xo), torch.from_numpy(mo), torch.from_numpy(vo), nb


def _expected(S, o, mode, lazy, wd, decay_1d, block=BLOCK0, advance=True):
    """every buffer after one launch, from the device's own o"""
    ins, k = S.ins, len(S.shapes)
    xs, ms, vs, es = [], [], [], []
    nb = None
    for i in range(k):
        xo, mo, vo, nb = _rule(ins["x"][i], o[i], ins["mom"][i], ins["v"][i], block, wd)
        xs.append(xo), ms.append(mo), vs.append(vo)
        es.append(ins["M"][i] if lazy else (ins["M"][i].double() - o[i].double()).float())
    want = {"x": S.ar.fill(xs), "M": S.ar.fill(es), "g": S.ar.fill(o if mode == 2 else ins["g"])}
    r1m, r1v = [], []
    if S.r1n:
        xo, mo, vo, nb = _rule(S.r1["x"], S.r1["buf"], S.r1["mom"], S.r1["v"], block, wd, float(S.q_div), decay_1d)
        r1m, r1v = [mo], [vo]
        want["r1x"] = S.ra.fill([xo])
        gg = S.r1["buf"] if S.q_div == 1 else torch.from_numpy(S.r1["buf"].numpy() / F(S.q_div))
        want["r1g"] = S.ra.fill([gg if mode == 2 else None])
    mo_all = S.host["mo"].clone()
    mo_all[: S.mv.total] = S.mv.fill(ms + r1m)
    mo_all[S.v_delta: S.v_delta + S.mv.total] = S.mv.fill(vs + r1v)
    want["mo"] = mo_all
    pp = S.host["pp"].clone()
    if lazy:
        pp[GUARD: GUARD + S.B.p_total] = _flat(S.B.p_offs, S.B.p_total, S.P)
    want["pp"] = pp
    want["comm"], want["qm"] = S.host["comm"], S.host["qm"]
    want["qw"] = _flat(S.B.q_offs, S.B.q_total, [(q.double() / S.q_div).float() for q in S.Qsum])
    b1, b2, steps = (float(nb[0]), float(nb[1]), nb[2]) if advance else (float(F(block[0])), float(F(block[1])), block[2])
    want["block"] = {"b1pow": b1, "b2pow": b2, "steps": steps}
    return want


def _check(snap, want, what):
    for nm, w in want.items():
        if nm == "block":
            assert snap["block"] == w, (what, snap["block"], w)
        else:
            _same(snap[nm], w, f"{what}: {nm}")
    assert not snap["ctr"].any(), f"{what}: the tickets were not re-armed"


@pytest.mark.parametrize("arm", R.ARMS)
@pytest.mark.parametrize("var", VARIANTS, ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("plan", PLANS)
def test_update_adam_stage(device, monkeypatch, plan, var, arm):
    mode, lazy, q_div, r1n, wd, decay_1d = var
    case = C.by_name(plan)
    assert all(n * m < C.MAX_ELEMS for n, m in case.shapes)
    B = _plan(case, device, monkeypatch)
    S = Setup(B, case.offs, arm, _gen("ua", plan, arm, *var), q_div, r1n, device)
    what = f"update_adam {plan} {arm} {var}"
    S.reset(wd=wd)
    S.launch(2, lazy, decay_1d)  # the mode-2 twin: the device's own o
    o = S.o_of(S.snapshot())
    # o against the stage rule
    worst = 0.0
    for i, ((n, m), r) in enumerate(zip(S.shapes, S.ranks)):
        res = R.update_stage(0, S.P[i], S.Qsum[i], float(q_div), M=S.ins["M"][i])
        if arm == "normal":
            Sabs = R.update_stage(0, S.P[i], S.Qsum[i], float(q_div), M=S.ins["M"][i], absolute=True)["out"]
            tol = (r + 1 + 8) * R.EPS32 * Sabs
            err = (o[i].double() - res["out"]).abs()
            assert bool((err <= tol).all()), f"{what}: o of matrix {i} off by {float((err - tol).max()):.3g} past its bound"
            live = tol > 0
            worst = max(worst, float((err[live] / tol[live]).max()))
        else:
            _same(o[i], res["out"], f"{what}: o of matrix {i}")
            if not lazy:  # e = M - out, exact arms: the rule's own
                _same((S.ins["M"][i].double() - o[i].double()).float(), res["mem"], f"{what}: e rule of matrix {i}")
    if arm == "normal":
        print(f"psgd-adam-ratio o {plan} {'-'.join(map(str, var))} {worst:.4f}")
    want = _expected(S, o, mode, lazy, wd, decay_1d)
    for attempt in ("first", "second"):  # the second launch finds the tickets re-armed
        S.reset(wd=wd)
        S.launch(mode, lazy, decay_1d)
        _check(S.snapshot(), want, f"{what} ({attempt})")


def test_special_values(device):
    """rows of o that are 1e-20, +inf, -inf and NaN, and a -0 parameter with g = m = v = 0 under wd = 0"""
    n, m, r = 8, 12, 4
    B = _PlanBuffers([(n, m)], r, 0, device)
    S = Setup(B, [0], "normal", _gen("ua-special"), 1, 0, device)
    vals = [1e-20, float("inf"), float("-inf"), float("nan"), 0.0, 3.0, -1e-20, 0.0]
    S.P[0] = torch.zeros(n, r)
    S.P[0][:, 0] = torch.tensor(vals)
    S.Qsum[0] = torch.zeros(m, r)
    S.Qsum[0][:, 0] = 1.0
    S.ins["x"][0][4] = -0.0
    S.ins["mom"][0][4] = 0.0
    S.ins["v"][0][4] = 0.0
    S.host["x"], S.host["comm"] = S.ar.fill(S.ins["x"]), _flat(B.p_offs, B.p_total, S.P)
    S.host["qm"] = _flat(B.q_offs, B.q_total, S.Qsum)
    mo = S.host["mo"]
    mo[: S.mv.total] = S.mv.fill(S.ins["mom"])
    mo[S.v_delta: S.v_delta + S.mv.total] = S.mv.fill(S.ins["v"])
    for wd in (0.0, WD):
        S.reset(wd=wd)
        S.launch(2, False, True)
        snap = S.snapshot()
        o = S.o_of(snap)[0]
        assert torch.all(o[0] == F(1e-20)) and torch.all(o[1] == float("inf")) and torch.all(o[2] == -float("inf"))
        assert torch.isnan(o[3]).all() and torch.all(o[4] == 0) and not torch.signbit(o[4]).any()
        xo, mo_, vo, _ = _rule(S.ins["x"][0], o, S.ins["mom"][0], S.ins["v"][0], BLOCK0, wd)
        s = S.ar.starts[0]
        assert A.same_bits(xo.numpy(), snap["x"][s: s + n * m].numpy()), wd
        ms = S.mv.starts[0]
        assert A.same_bits(mo_.numpy(), snap["mo"][ms: ms + n * m].numpy())
        assert A.same_bits(vo.numpy(), snap["mo"][S.v_delta + ms: S.v_delta + ms + n * m].numpy())
        with np.errstate(all="ignore"):
            e = S.ins["M"][0].numpy() - o.numpy()
        assert A.same_bits(e.ravel(), snap["M"][s: s + n * m].numpy())
        x4 = snap["x"][s: s + n * m].view(n, m)[4]
        if wd == 0.0:
            assert torch.all(x4 == 0) and torch.signbit(x4).all()  # the -0 survives
        assert torch.isnan(snap["x"][s: s + n * m].view(n, m)[3]).all()


def test_block_advances_once_over_several_launches(device, monkeypatch):
    """advance = 0, 0, 1 over disjoint item ranges: all three read the pre-step block, the result is one
    whole launch's bit for bit, steps goes up by one, the tickets end zero; and again on a second round"""
    case = C.by_name(PLANS[0])
    B = _plan(case, device, monkeypatch)
    S = Setup(B, case.offs, "normal", _gen("ua-block"), 4, 300, device)
    S.reset(wd=WD)
    snaps = []
    for _ in range(2):  # two rounds, the block carried over
        S.launch(2, False, False)
        snaps.append(S.snapshot())
    assert [s["block"]["steps"] for s in snaps] == [4, 5]
    S.reset(wd=WD)
    cuts = ((0, 2), (2, 5), (5, len(case.shapes)))
    for rnd in range(2):
        for j, (lo, hi) in enumerate(cuts):
            last = j == len(cuts) - 1
            S.launch(2, False, False, advance=last, items=B.items("u", lo, hi), r1=last)
            mid = S.snapshot()
            assert mid["block"]["steps"] == BLOCK0[2] + rnd + (1 if last else 0)
        got = S.snapshot()
        for nm in ("x", "mo", "M", "g", "r1x", "r1g", "qw", "pp"):
            _same(got[nm], snaps[rnd][nm], f"split launches, round {rnd}: {nm}")
        assert got["block"] == snaps[rnd]["block"] and not got["ctr"].any()


@pytest.mark.parametrize("arm", R.ARMS)
@pytest.mark.parametrize("numel", C.RANK1_SIZES)
@pytest.mark.parametrize("div,wd,decay_1d,write_g", [(4.0, WD, True, True), (1.0, WD, False, False), (4.0, 0.0, True, True)])
def test_rank1_adam_step_alone(device, numel, div, wd, decay_1d, write_g, arm):
    gen = _gen("r1a", numel, div, wd, arm)
    buf, mom, x = (R.stream(arm, gen, (numel,)) for _ in range(3))
    v = R.stream(arm, gen, (numel,)).abs()
    Ar = Arena([numel], [1])  # 4 bytes past a 16-byte boundary
    vd = _roundup(Ar.total, 4)
    mo = torch.full((2 * vd,), SENT)
    mo[: Ar.total] = Ar.fill([mom])
    mo[vd: vd + Ar.total] = Ar.fill([v])
    host = {"buf": Ar.fill([buf]), "x": Ar.fill([x]), "g": Ar.fill([None]), "mo": mo}
    dev = {k: t.to(device) for k, t in host.items()}
    sl = slice(Ar.starts[0], Ar.starts[0] + numel)
    block = StateBlock(device, ("b1pow", "b2pow", "steps"), BLOCK0)
    ctr = torch.zeros(ext().arrive_ctr_words(1024), dtype=torch.int32, device=device)
    hyper = torch.tensor([LR, wd, 0.0, 0.0], device=device)
    xo, mn, vn, nb = _rule(x, buf, mom, v, BLOCK0, wd, div, decay_1d)
    want_mo = mo.clone()
    want_mo[: Ar.total] = Ar.fill([mn])
    want_mo[vd: vd + Ar.total] = Ar.fill([vn])
    gg = buf if div == 1.0 else torch.from_numpy(buf.numpy() / F(div))
    for advance in (False, True, True):
        for k in host:
            dev[k].copy_(host[k])
        before = block.read()
        ext().rank1_adam_step(dev["buf"][sl], div, dev["mo"][sl], dev["x"][sl], dev["g"][sl] if write_g else None,
                              hyper, block.dev, ctr, dev["mo"], vd, BETAS[0], BETAS[1], EPS, decay_1d, advance)
        torch.cuda.synchronize()
        if before["steps"] == BLOCK0[2]:  # the scalars of BLOCK0: the rule above
            _same(dev["x"], Ar.fill([xo]), "x")
            _same(dev["mo"], want_mo, "moments")
            _same(dev["g"], Ar.fill([gg if write_g else None]), "g")
            _same(dev["buf"], host["buf"], "buf")
        after = block.read()
        assert after["steps"] == before["steps"] + int(advance) and not ctr.any()
    assert block.read() == {"b1pow": float(F(F(nb[0]) * F(BETAS[0]))), "b2pow": float(F(F(nb[1]) * F(BETAS[1]))),
                            "steps": BLOCK0[2] + 2}


def test_binding_refusals_launch_nothing(device, monkeypatch):
    case = C.by_name(PLANS[0])
    B = _plan(case, device, monkeypatch)
    S = Setup(B, case.offs, "int", _gen("ua-refuse"), 1, 300, device)
    S.reset()
    for mode in (0, 3):
        with pytest.raises(RuntimeError, match="modes 1 / 2"):
            S.launch(mode, False, True)
    with pytest.raises(RuntimeError, match="rank <= 16"):
        S.launch(1, False, True, max_rank=17)
    with pytest.raises(RuntimeError, match="AdamBlock is required"):
        S.launch(1, False, True, block=None)
    with pytest.raises(RuntimeError, match="hyper block"):
        S.launch(1, False, True, hyper=None)
    with pytest.raises(RuntimeError, match="tickets are required"):
        S.launch(1, False, True, ctr=None)
    with pytest.raises(RuntimeError, match="arrive_ctr_words"):
        S.launch(1, False, True, ctr=S.ctr[:64])
    with pytest.raises(RuntimeError, match="v_delta"):
        S.launch(1, False, True, v_delta=S.dev["mo"].numel())
    with pytest.raises(RuntimeError, match="betas"):
        S.launch(1, False, True, beta1=1.0)
    with pytest.raises(RuntimeError, match="eps"):
        S.launch(1, False, True, eps=0.0)
    T = _plan(C.by_name("taps-r4"), device, monkeypatch)  # refused before its (unbound) pointers could matter
    assert any(lay is not None for lay in T.layout)
    with pytest.raises(RuntimeError, match="dead-tap compacted"):
        ext().psgd_update_adam(T.geom, T.ptrs, T.u_items, T.comm_buf, T.q_memory, 1.0, T.q_warm, 1, T.max_rank,
                               geom_host=T._geom_host, hyper=S.hyper, block=S.block.dev, ctr=S.ctr, moments=S.dev["mo"],
                               v_delta=S.v_delta, beta1=BETAS[0], beta2=BETAS[1], eps=EPS, decay_1d=True, advance=True)
    torch.cuda.synchronize()
    snap = S.snapshot()
    for nm in ("x", "mo", "M", "g", "r1x", "pp"):
        _same(snap[nm], S.host[nm], f"after the refusals: {nm}")
    assert snap["block"]["steps"] == BLOCK0[2] and not snap["ctr"].any()
