"""Every PowerSGD P, Q and update kernel instance (csrc/powersgd.hip, csrc/plan.cpp) on its own against
the stage rules of tests/psgd_rule.py, for every case of tests/psgd_stage_cases.py and three input arms:

  int, mantissa   the rule is exact in fp32 (see psgd_rule.py): the device must be bitwise equal to it;
  normal          |dev - ref64| <= (K + 8) 2^-24 S per element, S the rule on absolute values, K the fp32
                  operations of the longest path (m + r + 2 for P, rows for Q, r + 6 for the update).

The driver builds _PlanBuffers directly, re-asserts the plan facts the case claims, binds MatPtrs rows
(API and engine form) that point into sentinel-filled arenas, writes the stage's inputs and launches the
stage alone: MGS is never in the path.  Every buffer the stage may write is compared whole, guard bands
included; every input it must not write has to come back bitwise; every stage runs twice from the same
state and must agree bitwise.  The largest err / bound of the normal arm is printed per run
("psgd-ratio ..."); profiles/r13/README.md records the maxima.
"""
import zlib

import pytest
import torch

from network_distributed_pytorch_amd.ops import SegPlan, ext
from network_distributed_pytorch_amd.parallel.powersgd import _PlanBuffers
from tests import psgd_rule as R
from tests import psgd_stage_cases as C

pytestmark = pytest.mark.gpu

SENT = 12345.0   # arena filler: finite, and nothing a rule produces
PRE = 7.0        # what an output buffer of the plan holds before the launch
GUARD = 64       # floats between two slots
_PLANS = {}


# ---- arenas ------------------------------------------------------------------------------------------
class Arena:
    """slots of ``sizes`` floats inside one sentinel-filled buffer; slot i starts ``offs[i]`` floats
    past a 16-byte boundary"""

    def __init__(self, sizes, offs=None):
        offs = offs or [0] * len(sizes)
        self.sizes, self.starts = list(sizes), []
        pos = GUARD
        for size, off in zip(sizes, offs):
            start = (pos + 3) // 4 * 4 + off
            self.starts.append(start)
            pos = start + size + GUARD
        self.total = pos

    def fill(self, tensors, dtype=torch.float32, base=SENT):
        """host buffer with ``tensors[i]`` (None: left at ``base``) in slot i"""
        buf = torch.full((self.total,), base, dtype=dtype)
        for s, n, t in zip(self.starts, self.sizes, tensors):
            if t is not None:
                assert t.numel() == n
                buf[s: s + n] = t.reshape(-1).to(dtype)
        return buf

    def ptr(self, dev, i):
        assert dev.data_ptr() % 256 == 0
        return dev.data_ptr() + 4 * self.starts[i]


def _flat(offs, total, tensors, dtype=torch.float32, base=SENT):
    """a flat plan buffer (P, Q layout): tensors[i] at offs[i]"""
    buf = torch.full((total,), base, dtype=dtype)
    for o, t in zip(offs, tensors):
        if t is not None:
            buf[o: o + t.numel()] = t.reshape(-1).to(dtype)
    return buf


class Expect:
    """reference, tolerance and the device tensor of every compared buffer"""

    def __init__(self):
        self.items = {}

    def add(self, name, dev, ref, tol=None):
        ref = ref.double()
        self.items[name] = (dev, ref, torch.zeros_like(ref) if tol is None else tol.double())

    def unchanged(self, name, dev, host):
        self.add(name, dev, host)

    def snapshot(self):
        return {k: dev.detach().cpu().clone() for k, (dev, _, _) in self.items.items()}

    def check(self, snap, what):
        worst = 0.0
        for k, (_, ref, tol) in self.items.items():
            got = snap[k].double()
            err = (got - ref).abs()
            bad = ~(err <= tol)
            if bad.any():
                i = int(bad.nonzero()[0])
                raise AssertionError(f"{what}: {k}[{i}] = {got[i].item()!r}, rule {ref[i].item()!r} +- {tol[i].item():.3g}"
                                     f" ({int(bad.sum())} of {bad.numel()} elements differ)")
            live = tol > 0
            if live.any():
                worst = max(worst, float((err[live] / tol[live]).max()))
        return worst


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32("/".join(map(str, key)).encode()))


def _bound(stage, n, m, r, S):
    return (R.k_ops(stage, n, m, r) + 8) * R.EPS32 * S


# ---- the plan ----------------------------------------------------------------------------------------
def _plan(case, device, monkeypatch):
    """_PlanBuffers of the case, built once under its NDP_PSGD_PKW; the claimed facts re-asserted"""
    if case.pkw is None:
        monkeypatch.delenv("NDP_PSGD_PKW", raising=False)
    else:
        monkeypatch.setenv("NDP_PSGD_PKW", str(case.pkw))
    B = _PLANS.get(case.name)
    if B is None:
        B = _PlanBuffers([tuple(s) for s in case.shapes], case.rank, C.R1_STRIDE + 300, device,
                         supports=[tuple(s) for s in case.supports] if case.supports else None)
        _PLANS[case.name] = B
    d = ext().build_plan([tuple(s) for s in case.shapes], case.rank,
                         [tuple(s) for s in case.supports] if case.supports else [])
    assert B.native and tuple(B.ranks) == case.ranks and B.max_rank == case.max_rank
    assert (B.p_cols, tuple(B.p_chunks), tuple(B.q_chunks), tuple(B.compact_cols)) == (
        case.p_cols, case.p_chunks, case.q_chunks, case.compact_cols), case.name
    assert tuple(d["q_rows"]) == case.q_rows and int(d["p_cols"]) == case.p_cols
    assert C.instances(B.max_rank, B.p_cols) == case.kernels
    assert [lay is not None for lay in B.layout] == [case.support(i) is not None for i in range(len(case.shapes))]
    return B


def _bind(B, rows):
    B._bind_key = None
    B.bind(rows, [B.vec_flag(i, row) for i, row in enumerate(rows)])


def _err_word(B):
    return int(B.orth_ctr[-1].item())


def _twice(launch, exp, what):
    """run ``launch`` twice from the same state: bitwise agreement, then the rule; -> err / bound"""
    launch()
    first = exp.snapshot()
    launch()
    second = exp.snapshot()
    for k in first:
        assert torch.equal(first[k], second[k]), f"{what}: {k} differs between two launches"
    return exp.check(first, what), first


# ---- P stage -----------------------------------------------------------------------------------------
def _p_inputs(case, arm, fuse):
    gen = _gen("p", case.name, arm, fuse)
    mats = []
    for i, ((n, m), r) in enumerate(zip(case.shapes, case.ranks)):
        sup = case.support(i)
        mc = case.compact_cols[i]
        g = R.stream(arm, gen, (n, m))
        if sup is None:
            Q = R.small_q(arm, gen, m, r, case.p_cols)
        else:
            g = R.expand(R.compress(g, *sup), m, *sup)  # exact zeros in the dead taps
            if arm == "mantissa" and r <= mc:  # the selector on live columns
                Q = torch.zeros(m, r)
                Q[R.full_columns(m, *sup)] = R.small_q(arm, gen, mc, r, max(1, case.p_cols * mc // m))
            else:
                Q = R.small_q(arm, gen, m, r, case.p_cols)
            if fuse == "prev":  # the rows of Q that dead columns of M produced
                Q = R.expand(R.compress(Q.t().contiguous(), *sup), m, *sup).t().contiguous()
        e = R.stream(arm, gen, (n, mc))
        pp = R.small_p_rows(arm, gen, n, r)
        mats.append(dict(g=g, Q=Q, e=e, pp=pp, sup=sup))
    return mats, R.stream(arm, gen, (300,))


def _p_rule(case, mats, arm, fuse, poked=False):
    """per matrix: P, its tolerance, the e slot afterwards (None: unchanged), its tolerance"""
    out = []
    for i, (mt, (n, m), r) in enumerate(zip(mats, case.shapes, case.ranks)):
        sup = mt["sup"]
        e = None if fuse == "off" else (mt["e"] if sup is None else R.expand(mt["e"], m, *sup))
        pp = mt["pp"] if fuse == "prev" else None
        P, M = R.p_stage(mt["g"], mt["Q"], e=e, p_prev=pp)
        tp = tm = None
        if arm == "normal":
            SP, SM = R.p_stage(mt["g"], mt["Q"], e=e, p_prev=pp, absolute=True)
            tp = _bound("p", n, m, r, SP)
            tm = None if SM is None else _bound("p", n, m, r, SM)
        else:
            assert torch.equal(P.float().double(), P)
        if M is not None and sup is not None:
            dead = torch.ones(m, dtype=torch.bool)
            dead[R.full_columns(m, *sup)] = False
            assert poked or not M[:, dead].any()  # the invariant the compact slot rests on
            M = R.compress(M, *sup)
            tm = None if tm is None else R.compress(tm, *sup)
        out.append((P, tp, M, tm))
    return out


def _run_p(case, arm, fuse, fused, device, monkeypatch, poke=None):
    B = _plan(case, device, monkeypatch)
    mats, r1 = _p_inputs(case, arm, fuse)
    if poke is not None:
        i, a, b = poke
        mats[i]["g"][a, b] = 2.0
    tapped_plan = case.supports is not None
    api = fuse == "off" and not tapped_plan
    G = Arena([n * m for n, m in case.shapes], case.offs)
    E = Arena([n * mc for (n, _), mc in zip(case.shapes, case.compact_cols)], case.offs)
    PP = Arena([B.p_total])
    g_host = G.fill([mt["g"] for mt in mats])
    e_host = E.fill([mt["e"] for mt in mats])
    pp_host = PP.fill([_flat(B.p_offs, B.p_total, [mt["pp"] for mt in mats])])
    qw_host = _flat(B.q_offs, B.q_total, [mt["Q"] for mt in mats])
    g_dev, e_dev, pp_dev = g_host.to(device), e_host.to(device), pp_host.to(device)
    r1_dev = r1.to(device)
    rows = []
    for i in range(len(mats)):
        gp, ep = G.ptr(g_dev, i), E.ptr(e_dev, i)
        rows.append([gp, 0, gp, 0, 0, 0, 0, 0] if api else [gp, ep, ep, 0, 0, 0, 0, gp])
    _bind(B, rows)
    pack = [(r1_dev, B.rank1_buf[:300], 1, 0, 1.0)]
    seg = SegPlan(pack, device)
    p_seg = SegPlan(B.p_seg_specs() + pack, device)
    p_prev = pp_dev[PP.starts[0]: PP.starts[0] + B.p_total] if fuse == "prev" else None

    rule = _p_rule(case, mats, arm, fuse, poked=poke is not None)
    exp = Expect()
    r1_ref = torch.full((B.r1_numel,), SENT)
    r1_ref[:300] = r1
    comm_ref = torch.cat([_flat(B.p_offs, B.p_total, [p for p, _, _, _ in rule], torch.float64), r1_ref.double()])
    comm_tol = torch.cat([_flat(B.p_offs, B.p_total, [t for _, t, _, _ in rule], torch.float64, 0.0),
                          torch.zeros(B.r1_numel, dtype=torch.float64)])
    exp.add("comm_buf", B.comm_buf, comm_ref, comm_tol)
    exp.add("e", e_dev, E.fill([mt["e"] if M is None else M for mt, (_, _, M, _) in zip(mats, rule)], torch.float64),
            E.fill([tm for _, _, _, tm in rule], torch.float64, 0.0))
    exp.unchanged("g", g_dev, g_host)
    exp.unchanged("q_warm", B.q_warm, qw_host)
    exp.unchanged("p_prev", pp_dev, pp_host)

    def launch(fused=fused):
        B.fused = fused
        B.comm_buf.fill_(SENT)
        B.p_part.fill_(SENT)
        B.q_warm.copy_(qw_host)
        e_dev.copy_(e_host)
        B.run_p(B.p_items, fuse != "off", p_prev, seg=seg, p_seg=p_seg)
        torch.cuda.synchronize()

    what = f"P {case.name} {arm} fuse_ef={fuse} fused={fused}"
    try:
        ratio, snap = _twice(launch, exp, what)
        if not fused and case.wide:  # the in-launch finish sums the same partials in the same order
            launch(True)
            other = exp.snapshot()
            for k in snap:
                assert torch.equal(snap[k], other[k]), f"{what}: {k} differs from the fused finish"
        assert _err_word(B) == (0 if poke is None else 2), what
    finally:
        B.fused = case.wide
        B.orth_ctr[-1] = 0
    return ratio


def _ids(runs):
    return [f"{c.name}-{'-'.join(map(str, v)) if isinstance(v, tuple) else v}" for _, c, v in runs]


P_RUNS = [x for x in C.stage_runs() if x[0] == "p"]
Q_RUNS = [x for x in C.stage_runs() if x[0] == "q"]
U_RUNS = [x for x in C.stage_runs() if x[0] == "u"]


@pytest.mark.parametrize("arm", R.ARMS)
@pytest.mark.parametrize("run", P_RUNS, ids=_ids(P_RUNS))
def test_p_stage(device, monkeypatch, run, arm):
    _, case, (fuse, fused) = run
    ratio = _run_p(case, arm, fuse, fused, device, monkeypatch)
    if arm == "normal":
        print(f"psgd-ratio p {case.kernels[0]} {case.name} {fuse} {fused} {ratio:.4f}")
        assert ratio <= 1.0


def test_dead_tap_gradient_sets_the_error_bit_alone(device, monkeypatch):
    """a nonzero gradient in a dead tap: bit 1 of the error word and no other bit; P still carries the
    full gradient, the compact slot the live columns (every buffer as the rule on the poked g)"""
    case = C.by_name("taps-r4")
    assert case.support(1) == (9, 1 << 4)
    _run_p(case, "int", "on", True, device, monkeypatch, poke=(1, 7, 9 * 60 + 2))


# ---- Q stage -----------------------------------------------------------------------------------------
def _run_q(case, arm, fused, device, monkeypatch):
    B = _plan(case, device, monkeypatch)
    gen = _gen("q", case.name, arm)
    tapped_plan = case.supports is not None
    Ms, Ps, q_ref, q_tol = [], [], [], []
    for i, ((n, m), r) in enumerate(zip(case.shapes, case.ranks)):
        sup = case.support(i)
        M = R.stream(arm, gen, (n, case.compact_cols[i]))
        P = R.small_p_cols(arm, gen, n, r, case.q_rows[i])
        Q = R.q_stage(M, P)
        tol = _bound("q", n, m, r, R.q_stage(M, P, absolute=True)) if arm == "normal" else torch.zeros_like(Q)
        if arm != "normal":
            assert torch.equal(Q.float().double(), Q)
        if sup is not None:
            # dead Q rows are never written by the kernel: they keep what the buffer held, or become the
            # sum of the (zero) partial rows where a seg_reduce finishes the matrix
            keep = PRE if fused and case.q_chunks[i] <= C.Q_FIN_MAX else 0.0
            Q = R.expand(Q.t().contiguous(), m, *sup, fill=keep).t().contiguous()
            tol = R.expand(tol.t().contiguous(), m, *sup).t().contiguous()
        Ms.append(M), Ps.append(P), q_ref.append(Q), q_tol.append(tol)
    E = Arena([M.numel() for M in Ms], case.offs)
    G = Arena([n * m for n, m in case.shapes], case.offs)
    e_host = E.fill(Ms)
    g_host = G.fill([None] * len(Ms))
    e_dev, g_dev = e_host.to(device), g_host.to(device)
    rows = []
    for i in range(len(Ms)):
        ep, gp = E.ptr(e_dev, i), G.ptr(g_dev, i)
        rows.append([gp, ep, ep, 0, 0, 0, 0, gp] if tapped_plan else [ep, 0, ep, 0, 0, 0, 0, 0])
    _bind(B, rows)
    comm_host = torch.cat([_flat(B.p_offs, B.p_total, Ps), torch.full((B.r1_numel,), SENT)])

    exp = Expect()
    exp.add("q_memory", B.q_memory, _flat(B.q_offs, B.q_total, q_ref, torch.float64),
            _flat(B.q_offs, B.q_total, q_tol, torch.float64, 0.0))
    exp.unchanged("comm_buf", B.comm_buf, comm_host)
    exp.unchanged("M", e_dev, e_host)
    exp.unchanged("g", g_dev, g_host)
    exp.unchanged("q_warm", B.q_warm, torch.full((B.q_total,), SENT))

    def launch(fused=fused):
        B.fused = fused
        B.comm_buf.copy_(comm_host)
        B.q_memory.fill_(PRE)
        B.q_warm.fill_(SENT)
        B.q_part.fill_(0.0 if tapped_plan else SENT)  # replan() zeroes the partials of a compacted plan
        B.run_q(B.q_items, B.q_seg)
        torch.cuda.synchronize()

    what = f"Q {case.name} {arm} fused={fused}"
    try:
        ratio, snap = _twice(launch, exp, what)
        if not fused and case.wide and not tapped_plan:
            launch(True)
            assert torch.equal(snap["q_memory"], exp.snapshot()["q_memory"]), f"{what}: differs from the fused finish"
        assert _err_word(B) == 0
    finally:
        B.fused = case.wide
    return ratio


@pytest.mark.parametrize("arm", R.ARMS)
@pytest.mark.parametrize("run", Q_RUNS, ids=_ids(Q_RUNS))
def test_q_stage(device, monkeypatch, run, arm):
    _, case, fused = run
    ratio = _run_q(case, arm, fused, device, monkeypatch)
    if arm == "normal":
        print(f"psgd-ratio q {case.kernels[1]} {case.name} {fused} {ratio:.4f}")
        assert ratio <= 1.0


# ---- update stage ------------------------------------------------------------------------------------
def _hyper(kind, device):
    """(hyper tensor or None, by-value lr, wd): with a block the by-value lr must be ignored"""
    if kind == "none":
        return None, R.LR, 0.0
    wd = R.WD if kind == "wd" else 0.0
    return torch.tensor([R.LR, wd, 0.0, 0.0], device=device), 99.0, wd


def _run_u(case, arm, var, device, monkeypatch):
    mode, lazy, hyper_kind, q_div, r1n = var
    B = _plan(case, device, monkeypatch)
    gen = _gen("u", case.name, arm, *var)
    hyper, lr_arg, wd = _hyper(hyper_kind, device)
    k = len(case.shapes)
    names = ("M", "mom", "x", "g", "out", "mem")
    ins = {nm: [] for nm in names}
    ref = {nm: [] for nm in names}
    tol = {nm: [] for nm in names}
    Ps, Qsums, qw_ref, qw_tol, pp_ref = [], [], [], [], []
    for i, ((n, m), r) in enumerate(zip(case.shapes, case.ranks)):
        sup = case.support(i)
        mc = case.compact_cols[i]
        P = R.small_p_rows(arm, gen, n, r)
        Qsum = R.stream(arm, gen, (m, r), 2) * (q_div if arm == "int" else 1)
        M, mom = R.stream(arm, gen, (n, mc)), R.stream(arm, gen, (n, mc))
        x, g = R.stream(arm, gen, (n, m)), R.stream(arm, gen, (n, m))
        cols = None if sup is None else R.full_columns(m, *sup)
        Ql = Qsum if sup is None else Qsum[cols]
        xl = x if sup is None else x[:, cols].contiguous()
        kw = dict(M=M, mom=mom, x=xl, lr=R.LR, momentum=R.MOMENTUM, wd=wd, lazy=lazy)
        res = R.update_stage(mode, P, Ql, float(q_div), **kw)
        S = R.update_stage(mode, P, Ql, float(q_div), absolute=True, **kw) if arm == "normal" else None
        warm = (Qsum.double() / q_div).float().double()  # Qs: every Q row, those of dead taps too
        assert sup is not None or torch.equal(warm, res["q_warm"])
        qw_ref.append(warm)
        qw_tol.append(None)  # one correctly rounded division in every arm
        pp_ref.append(P if lazy else None)
        if arm != "normal":
            for v in res.values():
                assert torch.equal(v.float().double(), v)

        def put(nm, inp, key, full_width=False):
            ins[nm].append(inp)
            if key not in res:
                ref[nm].append(None if inp is None else inp.double())
                tol[nm].append(None)
                return
            val = res[key]
            t = None if S is None else _bound("u", n, m, r, S[key])
            if full_width and sup is not None:  # live columns written, the dead ones untouched
                wide_val = inp.double().clone()
                wide_val[:, cols] = val
                val = wide_val
                if t is not None:
                    wt = torch.zeros(n, m, dtype=torch.float64)
                    wt[:, cols] = t
                    t = wt
            ref[nm].append(val)
            tol[nm].append(t)

        put("M", M, "e")
        put("mom", mom, "mom")
        put("x", x, "x", True)
        put("g", g, "g", True)
        put("out", None, "out")
        put("mem", None, "mem")
        Ps.append(P), Qsums.append(Qsum)

    full_sz = [n * m for n, m in case.shapes]
    comp_sz = [n * mc for (n, _), mc in zip(case.shapes, case.compact_cols)]
    arenas = {"M": Arena(comp_sz, case.offs), "mom": Arena(comp_sz, case.offs), "x": Arena(full_sz, case.offs),
              "g": Arena(full_sz, case.offs), "out": Arena(full_sz, case.offs), "mem": Arena(full_sz, case.offs)}
    host = {nm: arenas[nm].fill(ins[nm]) for nm in names}
    dev = {nm: host[nm].to(device) for nm in names}
    rows = []
    for i in range(k):
        p = {nm: arenas[nm].ptr(dev[nm], i) for nm in names}
        rows.append([p["M"], 0, p["M"], p["out"], p["mem"], 0, 0, 0] if mode == 0
                    else [p["g"], p["M"], p["M"], 0, 0, p["mom"], p["x"], p["g"]])
    _bind(B, rows)
    PP = Arena([B.p_total])
    pp_host = PP.fill([None])
    pp_dev = pp_host.to(device)
    p_prev = pp_dev[PP.starts[0]: PP.starts[0] + B.p_total] if lazy else None

    exp = Expect()
    for nm in names:
        exp.add(nm, dev[nm], arenas[nm].fill([host[nm][s: s + z] if v is None else v for v, s, z in
                                               zip(ref[nm], arenas[nm].starts, arenas[nm].sizes)], torch.float64),
                arenas[nm].fill(tol[nm], torch.float64, 0.0))
    exp.add("q_warm", B.q_warm, _flat(B.q_offs, B.q_total, qw_ref, torch.float64),
            _flat(B.q_offs, B.q_total, qw_tol, torch.float64, 0.0))
    exp.add("p_prev", pp_dev, PP.fill([_flat(B.p_offs, B.p_total, pp_ref, torch.float64)] if lazy else [None],
                                      torch.float64))
    qm_host = _flat(B.q_offs, B.q_total, Qsums)
    exp.unchanged("q_memory", B.q_memory, qm_host)

    # the rank-1 group stepped by the same call
    r1 = None
    r1_buf_host = torch.full((B.r1_numel,), SENT)
    if r1n:
        buf, rm, rx = (R.stream(arm, gen, (r1n,)) for _ in range(3))
        r1_buf_host[:r1n] = buf
        RA = Arena([r1n])
        r1_host = {"mom": RA.fill([rm]), "x": RA.fill([rx]), "g": RA.fill([None])}
        r1_dev = {nm: t.to(device) for nm, t in r1_host.items()}
        want = R.rank1_step(buf, float(q_div), rm, rx, R.LR, R.MOMENTUM, wd)
        S1 = R.rank1_step(buf, float(q_div), rm, rx, R.LR, R.MOMENTUM, wd, absolute=True)
        for nm in ("mom", "x", "g"):
            if nm == "g" and mode != 2:
                exp.unchanged("r1_g", r1_dev["g"], r1_host["g"])
                continue
            exp.add("r1_" + nm, r1_dev[nm], RA.fill([want[nm]], torch.float64),
                    RA.fill([_bound("r1", 0, 0, 0, S1[nm]) if arm == "normal" else None], torch.float64, 0.0))
        sl = slice(RA.starts[0], RA.starts[0] + r1n)
        r1 = dict(r1_buf=B.rank1_buf[:r1n], r1_div=float(q_div), r1_mom=r1_dev["mom"][sl], r1_x=r1_dev["x"][sl],
                  r1_g=r1_dev["g"][sl] if mode == 2 else None)
    comm_host = torch.cat([_flat(B.p_offs, B.p_total, Ps), r1_buf_host])
    exp.unchanged("comm_buf", B.comm_buf, comm_host)

    def launch():
        B.comm_buf.copy_(comm_host)
        B.q_memory.copy_(qm_host)
        B.q_warm.fill_(SENT)
        pp_dev.copy_(pp_host)
        for nm in names:
            dev[nm].copy_(host[nm])
        if r1 is not None:
            for nm in r1_host:
                r1_dev[nm].copy_(r1_host[nm])
        ext().psgd_update(B.geom, B.ptrs, B.u_items, B.comm_buf, B.q_memory, float(q_div), B.q_warm, mode, lr_arg,
                          R.MOMENTUM, B.max_rank, p_prev, hyper=hyper, **(r1 or {}))
        torch.cuda.synchronize()

    ratio, _ = _twice(launch, exp, f"update {case.name} {arm} {var}")
    assert _err_word(B) == 0
    return ratio


@pytest.mark.parametrize("arm", R.ARMS)
@pytest.mark.parametrize("run", U_RUNS, ids=_ids(U_RUNS))
def test_update_stage(device, monkeypatch, run, arm):
    _, case, var = run
    ratio = _run_u(case, arm, var, device, monkeypatch)
    if arm == "normal":
        print(f"psgd-ratio u {case.kernels[2]} {case.name} {'-'.join(map(str, var))} {ratio:.4f}")
        assert ratio <= 1.0


@pytest.mark.parametrize("arm", R.ARMS)
@pytest.mark.parametrize("hyper_kind,write_g", [("none", True), ("wd0", False), ("wd", True)])
@pytest.mark.parametrize("numel", C.RANK1_SIZES)
def test_rank1_step_alone(device, numel, hyper_kind, write_g, arm):
    gen = _gen("r1", numel, hyper_kind, arm)
    hyper, lr_arg, wd = _hyper(hyper_kind, device)
    buf, mom, x = (R.stream(arm, gen, (numel,)) for _ in range(3))
    A = Arena([numel], [1])  # 4 bytes past a 16-byte boundary
    host = {"buf": A.fill([buf]), "mom": A.fill([mom]), "x": A.fill([x]), "g": A.fill([None])}
    dev = {k: v.to(device) for k, v in host.items()}
    sl = slice(A.starts[0], A.starts[0] + numel)
    want = R.rank1_step(buf, 4.0, mom, x, R.LR, R.MOMENTUM, wd)
    S = R.rank1_step(buf, 4.0, mom, x, R.LR, R.MOMENTUM, wd, absolute=True)
    exp = Expect()
    exp.unchanged("buf", dev["buf"], host["buf"])
    for nm in ("mom", "x", "g"):
        if nm == "g" and not write_g:
            exp.unchanged("g", dev["g"], host["g"])
            continue
        exp.add(nm, dev[nm], A.fill([want[nm]], torch.float64),
                A.fill([_bound("r1", 0, 0, 0, S[nm]) if arm == "normal" else None], torch.float64, 0.0))

    def launch():
        for k in host:
            dev[k].copy_(host[k])
        ext().rank1_step(dev["buf"][sl], 4.0, dev["mom"][sl], dev["x"][sl], dev["g"][sl] if write_g else None, lr_arg,
                         R.MOMENTUM, hyper=hyper)
        torch.cuda.synchronize()

    ratio, _ = _twice(launch, exp, f"rank1_step {numel} {hyper_kind} {arm}")
    if arm == "normal":
        print(f"psgd-ratio r1 rank1_step {numel} {hyper_kind} {ratio:.4f}")
        assert ratio <= 1.0
