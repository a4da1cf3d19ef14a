"""Every DistilBERT kernel instance and launch geometry (csrc/layernorm.hip, attention.hip, linear.hip,
embedding.hip), one test per case of tests/bert_kernel_cases.py, through the bindings ln_fwd / ln_bwd,
attn_fwd / attn_bwd, colsum, gelu_bwd_colsum, embedding_backward and slab_sum, so that every output and
scratch buffer is the test's own and starts as NaN: an element that no workgroup writes fails.  (The
embedding's row_cnt starts zeroed, as at allocation; its int32 perm starts as T, the index of a NaN row
kept behind grad_out, and row_start as 0: a stale entry is only ever used as an address, so the poison
must stay in bounds.)  Inputs are compared with their host originals at the end of each case.

The references are tests/bert_rule.py's: fp64 rules and, where a sum is pure additions, its exact fp32
order.  Where the launch geometry decides the result, the case first asserts that the extension's
colsum_chunks / ln_bwd_wgs equal the twins.

Bounds (none is new):
  LayerNorm   tests/test_layernorm_gpu.py: y rtol 1e-5, atol 2e-5 (3e-5 with dropout); dx / da rtol 1e-4,
              the same atol; dgamma / dbeta rtol 1e-4, atol that * sqrt(R).  s gets y's bound; mean and
              rstd rtol 1e-5 against the fp64 statistics of the kernel's fp32 s.
  attention   tests/test_attention.py _check: err <= tol * max|ref| + 1e-6 with tol 2e-5 forward (o, and
              delta against fp64 rowsum(dO * O)) and 5e-5 backward (dq, dk, dv).  lse: m + log l against
              the fp64 logsumexp, 2e-5 * max(1, |ref|); fully padded rows m == finfo.min exactly and
              log l within 1e-5 of log S.
  column sums tests/test_linear_gpu.py: 1e-5 * max(1, max|ref|) * sqrt(M).
  GELU dh     twice the error of ATen's own fp32 gelu_backward on the same inputs against the same fp64
              reference (the same formula with another libm: one more rounding in erf and exp each), plus
              one fp32 ulp of max|ref|.  Figures in profiles/r14/README.md.
  embedding   bitwise against the token-order sum.
For the rtol / atol bounds the printed err is max(|got - ref| - rtol * |ref|), judged against atol; for
mean and rstd it is max(|got - ref| / |ref|), judged against rtol.

With a single key the softmax is 1 whatever the score, so dq and dk are identically zero, max|ref| is 0 and
their bound is its 1e-6 floor alone, while the kernels form p * (dP / (1 - p) - delta) from two separately
rounded sums of magnitude |dO . V| (up to 11 here, one fp32 ulp of which is 9.5e-07).  With delta summed in
fp32 the S = 1 case with dropout missed that floor (dq err 1.045e-06); attn_bwd_delta_kernel now sums in
double and the case gives 8.36e-07 (dk 5.25e-07), the rounding of the MFMA chain behind dP alone.

Every figure is printed before it is judged ("BERTERR <case> <quantity> err scale bound"); a case collects
all of its failed checks before it asserts.  The per-family maxima are in profiles/r14/README.md.
"""
import math
import zlib

import pytest
import torch

from network_distributed_pytorch_amd.ops import ext
from tests import bert_kernel_cases as C
from tests import bert_rule as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
EPS = 1e-12   # DistilBERT's LayerNorm eps


class _Report:
    """collects every failed check of a case, so that one run shows them all"""

    def __init__(self, case):
        self.case, self.bad = case, []

    def true(self, name, ok, detail=""):
        if not ok:
            self.bad.append(f"{name} {detail}".strip())

    def same(self, name, a, b):
        if not (a.shape == b.shape and torch.equal(a, b)):
            n = (a != b).sum().item() if a.shape == b.shape else -1
            self.bad.append(f"{name}: not bitwise equal ({n} of {a.numel()} elements differ)")

    def figure(self, name, err, scale, bound):
        print(f"BERTERR {self.case.id} {name} err {err:.3e} scale {scale:.3e} bound {bound:.3e}")
        if not err <= bound:  # (a NaN fails)
            self.bad.append(f"{name}: err {err:.3e} > bound {bound:.3e} (scale {scale:.3e})")

    def close(self, name, got, ref, rtol, atol):
        """|got - ref| <= atol + rtol * |ref| for every element"""
        if got.numel() == 0:
            return
        ref = ref.double().reshape(got.shape)
        d = (got.double() - ref).abs() - rtol * ref.abs()
        d = torch.where(torch.isnan(d), torch.full_like(d, math.inf), d)
        self.figure(name, d.max().item(), ref.abs().max().item(), atol)

    def rel(self, name, got, ref, rtol):
        """|got - ref| <= rtol * |ref| for every element (ref nowhere zero)"""
        ref = ref.double().reshape(got.shape)
        d = (got.double() - ref).abs() / ref.abs()
        d = torch.where(torch.isnan(d), torch.full_like(d, math.inf), d)
        self.figure(name, d.max().item(), ref.abs().min().item(), rtol)

    def scaled(self, name, got, ref, tol, floor=0.0):
        """max|got - ref| <= tol * max|ref| + floor"""
        ref = ref.double().reshape(got.shape)
        d = (got.double() - ref).abs()
        d = torch.where(torch.isnan(d), torch.full_like(d, math.inf), d)
        scale = ref.abs().max().item()
        self.figure(name, d.max().item(), scale, tol * scale + floor)

    def done(self):
        assert not self.bad, f"{self.case.id}:\n  " + "\n  ".join(self.bad)


def _nan(shape, device, dtype=torch.float32):
    return torch.full(tuple(shape), NAN, device=device, dtype=dtype)


def _gen(case, tag=""):
    return torch.Generator().manual_seed(zlib.crc32(f"{case.id}/{tag}".encode()))


def _unchanged(rep, dev, host):
    for name, t in host.items():
        if t is not None:
            rep.same(f"input {name} unchanged", dev[name].cpu(), t)


# ------------------------------------------------ LayerNorm ------------------------------------------------
def _ln_run(X, case, d, seed, deferred):
    Rr, D, dev = case.R, case.D, d["a"].device
    o = dict(y=_nan((Rr, D), dev), s=_nan((Rr, D), dev), mean=_nan((Rr,), dev), rstd=_nan((Rr,), dev),
             dx=_nan((Rr, D), dev), dgb=_nan((2 * D,), dev))
    X.ln_fwd(d["a"], d["b"], d["gamma"], d["beta"], o["y"], o["s"], o["mean"], o["rstd"], EPS, case.mode, case.p,
             seed)
    o["da"] = _nan((Rr, D), dev) if case.mode == 1 else None
    o["part"] = _nan((R.ln_bwd_wgs(Rr) * 2 * D,), dev) if deferred else None
    o["left"] = X.ln_bwd(d["dy"], o["s"], o["mean"], o["rstd"], d["gamma"], o["dx"], o["dgb"], case.mode, case.p,
                         seed, o["da"], o["part"])
    return o


@pytest.mark.parametrize("case", C.ln_cases(), ids=lambda c: c.id)
def test_layernorm_case(device, case):
    X, rep = ext(), _Report(case)
    Rr, D, mode, p = case.R, case.D, case.mode, case.p
    g = _gen(case)
    # rows centred well away from zero, so that the relative bound on the saved mean is one on its error
    host = dict(a=torch.randn(Rr, D, generator=g) * 2 + 3, b=torch.randn(Rr, D, generator=g) if case.res else None,
                gamma=torch.rand(D, generator=g) + 0.5, beta=torch.rand(D, generator=g) - 0.5,
                dy=torch.randn(Rr, D, generator=g))
    d = {k: (v.to(device) if v is not None else None) for k, v in host.items()}
    seed = torch.tensor([case.seed], dtype=torch.int32, device=device) if mode else None
    keep = R.ln_keep(case.seed, Rr, D, p, device) if mode else None
    ref = R.add_ln_rule(d["a"], d["b"], d["gamma"], d["beta"], EPS, mode, keep, p, d["dy"])
    wgs = R.ln_bwd_wgs(Rr)
    assert X.ln_bwd_wgs(Rr) == wgs

    o = _ln_run(X, case, d, seed, False)
    rep.true("plain ln_bwd returns 0", o["left"] == 0, str(o["left"]))
    atol = 3e-5 if mode else 2e-5
    rep.close("y", o["y"], ref["y"], 1e-5, atol)
    rep.close("s", o["s"], ref["s"], 1e-5, atol)
    s64 = o["s"].double()
    mean64 = s64.mean(-1)
    rstd64 = 1.0 / torch.sqrt(((s64 - mean64[:, None]) ** 2).mean(-1) + EPS)
    rep.rel("mean", o["mean"], mean64, 1e-5)   # (the printed scale is min|ref|)
    rep.rel("rstd", o["rstd"], rstd64, 1e-5)
    rep.close("dx", o["dx"], ref["dx"], 1e-4, atol)
    if mode == 1:
        rep.close("da", o["da"], ref["da"], 1e-4, atol)
        rep.true("da of dropped elements is exactly 0", not o["da"][~keep].any().item())
    if mode == 2:
        rep.true("y of dropped elements is exactly 0", not o["y"][~keep].any().item())
    rep.close("dgamma", o["dgb"][:D], ref["dgamma"], 1e-4, atol * Rr ** 0.5)
    rep.close("dbeta", o["dgb"][D:], ref["dbeta"], 1e-4, atol * Rr ** 0.5)
    if mode != 2:  # dbeta is pure additions of dy
        rep.same("dbeta in the kernel's order", o["dgb"][D:], R.ln_dbeta_order(d["dy"]))
    if case.gap:
        row, col = case.gap
        rep.true("the rule keeps the gap element", bool(keep[row, col]))
        t = o["da"] if mode == 1 else o["y"]
        rep.true("the kernel keeps the gap element (double threshold)", t[row, col].item() != 0.0)

    o2 = _ln_run(X, case, d, seed, False)
    for k in ("y", "s", "mean", "rstd", "dx", "da", "dgb"):
        if o[k] is not None:
            rep.same(f"second run {k}", o2[k], o[k])

    if case.deferred:
        o3 = _ln_run(X, case, d, seed, True)
        rep.true("deferred ln_bwd returns its workgroup count", o3["left"] == wgs, f"{o3['left']} != {wgs}")
        rep.true("deferred dgb untouched", torch.isnan(o3["dgb"]).all().item())
        rep.true("deferred partials all written", not torch.isnan(o3["part"]).any().item())
        for k in ("dx", "da"):
            if o[k] is not None:
                rep.same(f"deferred {k}", o3[k], o[k])
        if wgs >= 2:
            dgb = _nan((2 * D,), device)
            X.slab_sum(o3["part"], dgb, wgs)
            rep.same("deferred partials summed by slab_sum", dgb, o["dgb"])
        else:
            rep.same("the single deferred partial", o3["part"], o["dgb"])
        if mode != 2:
            rep.same("dbeta partials in the kernel's order", o3["part"].view(wgs, 2 * D)[:, D:],
                     R.ln_dbeta_partials_order(d["dy"]))
    _unchanged(rep, d, host)
    rep.done()


# ------------------------------------------------ attention ------------------------------------------------
def _attn_run(X, case, d, mask, seed, packed):
    """o, lse, delta, dq, dk, dv of one forward + backward; packed: q / k / v and their gradients are
    views into [B, S, 3, H, 64] buffers (token stride 3 * H * 64)"""
    B, S, H, dev = case.B, case.S, case.H, d["q"].device
    if packed:
        buf = _nan((B, S, 3, H, 64), dev)
        for i, n in enumerate("qkv"):
            buf[:, :, i].copy_(d[n])
        q, k, v = (buf[:, :, i] for i in range(3))
        gbuf = _nan((B, S, 3, H, 64), dev)
        dq, dk, dv = (gbuf[:, :, i] for i in range(3))
    else:
        q, k, v = d["q"], d["k"], d["v"]
        dq, dk, dv = (_nan((B, S, H, 64), dev) for _ in range(3))
    o, lse, delta = _nan((B, S, H, 64), dev), _nan((2, B, H, S), dev), _nan((B, H, S), dev)
    scale = 1.0 / math.sqrt(64)
    X.attn_fwd(q, k, v, mask, o, lse, scale, seed, case.p)
    X.attn_bwd(q, k, v, mask, o, d["dout"], lse, delta, dq, dk, dv, scale, seed, case.p)
    return dict(o=o, lse=lse, delta=delta, dq=dq.contiguous(), dk=dk.contiguous(), dv=dv.contiguous())


@pytest.mark.parametrize("case", C.attn_cases(), ids=lambda c: c.id)
def test_attention_case(device, case):
    X, rep = ext(), _Report(case)
    B, S, H, p = case.B, case.S, case.H, case.p
    g = _gen(case)
    host = {n: torch.randn(B, S, H, 64, generator=g) for n in ("q", "k", "v", "dout")}
    rows = C.attn_mask(case)
    host["mask"] = torch.tensor(rows, dtype=torch.int32) if rows is not None else None
    d = {k: (v.to(device) if v is not None else None) for k, v in host.items()}
    mask = d["mask"]
    seed = torch.tensor([case.seed], dtype=torch.int32, device=device) if p > 0 else None
    keep = R.attn_keep(case.seed, B * H, S, p, device) if p > 0 else None
    ref = R.attention_rule(d["q"], d["k"], d["v"], mask, keep, p, d["dout"])
    if case.gap:
        bh, qi, ki = case.gap
        rep.true("the rule keeps the gap element", bool(keep[bh, qi, ki]))
    del keep

    o = _attn_run(X, case, d, mask, seed, case.packed)
    rep.scaled("o", o["o"], ref["o"], 2e-5, 1e-6)
    rep.scaled("delta", o["delta"], ref["delta"], 2e-5, 1e-6)
    for n in ("dq", "dk", "dv"):
        rep.scaled(n, o[n], ref[n], 5e-5, 1e-6)
    # lse: [2][B, H, S] = row max m, then log l
    m, logl = o["lse"][0], o["lse"][1]
    live = torch.ones(B, dtype=torch.bool, device=device) if mask is None else (mask != 0).any(1)
    if live.any():
        got = m[live].double() + logl[live].double()
        want = ref["m"][live] + ref["logl"][live]
        e = ((got - want).abs() / want.abs().clamp(min=1.0))
        e = torch.where(torch.isnan(e), torch.full_like(e, math.inf), e)
        rep.figure("lse", e.max().item(), want.abs().max().item(), 2e-5)
    if not live.all():
        rep.true("m of fully padded rows is finfo.min", (m[~live] == R.F32_MIN).all().item())
        e = (logl[~live].double() - math.log(S)).abs()
        e = torch.where(torch.isnan(e), torch.full_like(e, math.inf), e)
        rep.figure("log l of fully padded rows", e.max().item(), math.log(S), 1e-5)
    if mask is not None:
        dead = mask == 0                                    # [B, S] masked keys
        rep.true("dk of masked keys is exactly 0", not o["dk"][dead].any().item())
        dead_live = dead & live[:, None]                    # ... of batch rows that attend to some key
        rep.true("dv of masked keys is exactly 0", not o["dv"][dead_live].any().item())

    o2 = _attn_run(X, case, d, mask, seed, case.packed)
    for n in o:
        rep.same(f"second run {n}", o2[n], o[n])
    if case.packed:
        o3 = _attn_run(X, case, d, mask, seed, False)
        for n in o:
            rep.same(f"contiguous {n} equals packed", o3[n], o[n])
    _unchanged(rep, d, host)
    rep.done()


# ---------------------------------------- column sums, GELU backward ---------------------------------------
@pytest.mark.parametrize("case", C.col_cases(), ids=lambda c: c.id)
def test_colsum_case(device, case):
    X, rep = ext(), _Report(case)
    M, N = case.M, case.N
    host = dict(g=torch.randn(M, N, generator=_gen(case)))
    d = {k: v.to(device) for k, v in host.items()}
    chunks = R.colsum_chunks(M, N)
    assert X.colsum_chunks(M, N) == chunks

    out = _nan((N,), device)
    rep.true("plain colsum returns 0", X.colsum(d["g"], out, None) == 0)
    rep.same("out in the kernel's order", out, R.colsum_order(d["g"]))
    ref = R.colsum_rule(d["g"])
    rep.figure("out", (out.double() - ref).abs().max().item(), ref.abs().max().item(),
               1e-5 * max(1.0, ref.abs().max().item()) * M ** 0.5)

    out2, part = _nan((N,), device), _nan((chunks * N,), device)
    left = X.colsum(d["g"], out2, part)
    rep.true("deferred colsum returns its chunk count", left == chunks, f"{left} != {chunks}")
    rep.true("deferred out untouched", torch.isnan(out2).all().item())
    rep.same("partials in the kernel's order", part.view(chunks, N), R.colsum_partials_order(d["g"]))
    rep.same("partials summed in order", R.slab_sum_order(part, chunks, N), out)
    _unchanged(rep, d, host)
    rep.done()


def _ulp(x: float) -> float:
    """the spacing of fp32 at |x|"""
    t = torch.tensor(abs(x), dtype=torch.float32)
    return (torch.nextafter(t, torch.tensor(math.inf)) - t).item()


@pytest.mark.parametrize("case", C.col_cases(), ids=lambda c: c.id)
def test_gelu_bwd_colsum_case(device, case):
    X, rep = ext(), _Report(case)
    M, N = case.M, case.N
    gen = _gen(case, "gelu")
    host = dict(g=torch.randn(M, N, generator=gen), h=torch.randn(M, N, generator=gen) * 2)
    ns = min(len(C.GELU_SPECIALS), M * N)
    host["h"].view(-1)[:ns] = torch.tensor(C.GELU_SPECIALS[:ns])
    d = {k: v.to(device) for k, v in host.items()}
    chunks = R.colsum_chunks(M, N)
    assert X.colsum_chunks(M, N) == chunks

    dh, db = _nan((M, N), device), _nan((N,), device)
    rep.true("plain gelu_bwd_colsum returns 0", X.gelu_bwd_colsum(d["g"], d["h"], dh, db, None) == 0)
    rep.same("db is the kernel's dh in the kernel's order", db, R.colsum_order(dh))
    ref = R.gelu_bwd_rule(d["g"], d["h"])
    aten = torch.ops.aten.gelu_backward(d["g"], d["h"], approximate="none")
    err_aten = (aten.double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    bound = 2.0 * err_aten + _ulp(scale)
    print(f"BERTERR {case.id} dh-aten err {err_aten:.3e} scale {scale:.3e} bound -")
    e = (dh.double() - ref).abs()
    e = torch.where(torch.isnan(e), torch.full_like(e, math.inf), e)
    rep.figure("dh", e.max().item(), scale, bound)
    sp_dh, sp_g, sp_h = dh.view(-1)[:ns], d["g"].view(-1)[:ns], d["h"].view(-1)[:ns]
    rep.true("dh finite at the special inputs", torch.isfinite(sp_dh).all().item(), str(sp_dh.tolist()))
    zero = sp_h == 0
    ez = (sp_dh[zero].double() - sp_g[zero].double() * 0.5).abs().max().item()
    rep.figure("dh at h = +-0 against g / 2", ez, scale, bound)

    dh2, db2, part = _nan((M, N), device), _nan((N,), device), _nan((chunks * N,), device)
    left = X.gelu_bwd_colsum(d["g"], d["h"], dh2, db2, part)
    rep.true("deferred gelu_bwd_colsum returns its chunk count", left == chunks, f"{left} != {chunks}")
    rep.true("deferred db untouched", torch.isnan(db2).all().item())
    rep.same("deferred dh", dh2, dh)
    rep.same("partials in the kernel's order", part.view(chunks, N), R.colsum_partials_order(dh))
    rep.same("partials summed in order", R.slab_sum_order(part, chunks, N), db)
    _unchanged(rep, d, host)
    rep.done()


# ------------------------------------------------ embedding ------------------------------------------------
def _emb_call(X, case, ids, scratch, gen, device):
    """one embedding_backward on the shared scratch: gw, and grad_out (a view that ends before a NaN row)"""
    T, V, D = case.T, case.V, case.D
    buf = _nan((T + 1, D), device)
    buf[:T] = torch.randn(T, D, generator=gen).to(device)
    gout, gw = buf[:T], _nan((V, D), device)
    X.embedding_backward(ids, gout, gw, -1 if case.pad is None else case.pad, *scratch)
    return gw, gout


@pytest.mark.parametrize("case", C.emb_cases(), ids=lambda c: c.id)
def test_embedding_backward_case(device, case):
    X, rep = ext(), _Report(case)
    T, V, D = case.T, case.V, case.D
    gen = _gen(case)
    perm = torch.full((max(T, 1),), T, dtype=torch.int32, device=device)  # a stale entry reads the NaN row
    row_start = torch.zeros(V, dtype=torch.int32, device=device)
    row_cnt = torch.zeros(V, dtype=torch.int32, device=device)             # zeroed, as at allocation
    scratch = (perm, row_start, row_cnt)
    for call in (0, 1):   # the second call, with other ids, runs on what the first left in the scratch
        host_ids = C.emb_ids(case, call)
        ids = host_ids.to(device)
        gw, gout = _emb_call(X, case, ids, scratch, gen, device)
        want = R.embedding_bwd_order(ids, gout, V, case.pad)
        rep.same(f"call {call}: gw is the token-order sum", gw, want)
        rep.true(f"call {call}: row_cnt re-armed", not row_cnt.any().item())
        ref = R.embedding_bwd_rule(ids, gout, V, case.pad)
        rep.figure(f"call{call}-order-vs-fp64", (want.double() - ref).abs().max().item() if V * D else 0.0,
                   ref.abs().max().item(), 1e-5 * max(1.0, ref.abs().max().item()))  # tests/test_embedding_gpu.py
        if T == 0:
            rep.true(f"call {call}: no tokens, gw all zero", not gw.any().item() and not torch.isnan(gw).any().item())
        if case.pad is not None:
            rep.true(f"call {call}: the padding row is zero", not gw[case.pad].any().item())
        rep.same(f"call {call}: ids unchanged", ids.cpu(), host_ids)
    rep.done()
