"""Every distinct direct-conv plan of csrc/conv.hip, csrc/winograd.hip and csrc/ds_stream.h against an
fp64 oracle, through the bindings, with every launch option that the plan allows.

tests/conv_plan_cases.py lists at most two batches per plan key of the recorded table
(tests/golden/conv_plan_table.json); tests/test_conv_plan_cases_cpu.py pins that the list leaves no
key out.  Each case here sets the case's switches, asserts that conv_plan, conv_stats_slices,
conv_dgrad_stats_slices and conv_wino report the case's row (so the launches below cannot silently
take another route), and then runs conv_fwd, conv_dgrad and conv_wgrad the way ops/conv.py calls
them: plain, with the split-K slabs left to the consumer (defer), with the BatchNorm statistics
epilogues (forward; backward with and without an addend), grad-x with an addend, grad-W with and
without its slab sum, and the backward pair (grad-W held back for the grad-x launch).  Outputs and
scratch are pre-filled with NaN, so an element that no workgroup writes fails.

What is compared with what:
  * y, dx, dx + addend and dw with float64 F.conv2d and its autograd on the CPU, computed once per
    (geometry, batch) and shared by both switch values and every option.  Bounds are the project's
    own: a direct kernel err <= 2e-6 * max|ref| * sqrt(C * KH * KW) + 1e-6 (test_direct_conv_vs_fp64),
    a direction that runs a Winograd kernel err <= 4e-6 * sqrt(9 * C) * max|ref|
    (test_winograd_vs_direct_vs_fp64; layer1's grad-W is a Winograd kernel while the switch is on).
  * everything else bitwise: a second run, wino_u built by the binding, y / dx with a statistics
    epilogue, the slabs a deferred launch leaves (summed by _slab_sum in the order of
    conv_slab_sum_kernel, the addend last), the grad-W slabs, the odd pixels of a 1x1 stride-2
    grad-x with an addend, and the pair launch against the two launches alone.
  * the statistics partials with fp64 sums, with the tolerances of tests/test_conv_bnstats_gpu.py.

The backward pair counts one pair launch where launch_conv_wgrad holds the grad-W back and the
grad-x launch can take it: the 3x3 classes when their grad-x is a Winograd launch (layer1 and
kConv3x3Map4 at every batch, kConv3x3S2 up to batch 256) and the 1x1 stride-2 classes always.
Layer1 also holds its Winograd grad-W when the grad-x is direct (batches below the Winograd
threshold); the grad-x then launches it alone and the counter stays.

Every figure is printed before it is judged ("PLANERR <case> <direction> <kernel> err scale bound");
the per-class maxima are recorded in profiles/r12/README.md.
"""
import zlib

import pytest
import torch
import torch.nn.functional as F

from tests import conv_plan_cases as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
CASES = R.cases()
UPS = (4, 5)    # the 1x1 stride-2 classes: compact grad-x slabs, no deferral
STEM_CLS = 3
_DATA: dict = {}  # (geometry index, batch) -> operands and reference; R.cases() keeps sharers adjacent


def _data(case, device):
    """Seeded x, w, dy, addend (and the consuming BN's x, y, mean, invstd where a grad-x emits
    statistics) on the device, their host originals, and the fp64 y, dx, dw: once per (geometry,
    batch), never modified.  One entry is kept: the next (geometry, batch) replaces it."""
    key = (case.gi, case.B)
    if key not in _DATA:
        _DATA.clear()
        C, H, W, Co, KH, KW, s, p = case.geom
        B = case.B
        OH, OW = (H + 2 * p - KH) // s + 1, (W + 2 * p - KW) // s + 1
        g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
        host = dict(x=torch.randn(B, C, H, W, generator=g),
                    w=torch.randn(Co, C, KH, KW, generator=g) / (C * KH * KW) ** 0.5,
                    dy=torch.randn(B, Co, OH, OW, generator=g),
                    add=torch.randn(B, C, H, W, generator=g))
        if case.cls in (0, 2):  # the classes whose grad-x has the backward statistics epilogue
            host.update(bx=torch.randn(B, C, H, W, generator=g) * 1.5 + 0.2,
                        by=torch.relu(torch.randn(B, C, H, W, generator=g)),
                        mean=torch.randn(C, generator=g) * 0.1, invstd=torch.rand(C, generator=g) + 0.5)
        xd = host["x"].double().requires_grad_(case.cls != STEM_CLS)  # the stem's input needs no gradient
        wd = host["w"].double().requires_grad_(True)
        y = F.conv2d(xd, wd, stride=s, padding=p)
        y.backward(host["dy"].double())
        d = {k: v.to(device) for k, v in host.items()}
        d["host"] = host
        d["ref"] = dict(y=y.detach().to(device), dw=wd.grad.to(device),
                        dx=xd.grad.to(device) if xd.grad is not None else None)
        _DATA[key] = d
    return _DATA[key]


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

    def close(self, name, got, ref, wino):
        """the project's fp64 bounds (module docstring)"""
        C, _H, _W, _Co, KH, KW, _s, _p = self.case.geom
        err = (got.double() - ref).abs().max().item()
        scale = ref.abs().max().item()
        bound = 4e-6 * (9 * C) ** 0.5 * scale if wino else 2e-6 * scale * (C * KH * KW) ** 0.5 + 1e-6
        print(f"PLANERR {self.case.id} {name} {'winograd' if wino else 'direct'} err {err:.3e} scale {scale:.3e} "
              f"bound {bound:.3e}")
        if not err <= bound:  # (a NaN fails)
            self.bad.append(f"{name}: err {err:.3e} > bound {bound:.3e} (scale {scale:.3e})")


def _nan(shape, device, dtype=torch.float32):
    return torch.full(tuple(shape), NAN, device=device, dtype=dtype)


def _slab_sum(part, n, numel, addend=None):
    """The fp32 sum of n slabs in the order of conv_slab_sum_kernel: group g adds slabs g, g + 16, ...
    onto zero, the 16 groups are added in order, the addend last (n <= 16: plain slab order)."""
    s = part[: n * numel].view(n, numel)
    acc = torch.zeros(min(n, 16), numel, device=part.device)
    for j in range(0, n, 16):
        chunk = s[j: j + 16]
        acc[: chunk.shape[0]] += chunk
    t = acc[0].clone()
    for k in range(1, acc.shape[0]):
        t += acc[k]
    if addend is not None:
        t += addend.reshape(-1)
    return t


def _assert_plan(X, case):
    geom = list(case.geom)
    got = tuple(int(v) for v in X.conv_plan(geom, case.B)) + (
        int(X.conv_stats_slices(geom, case.B)), int(X.conv_dgrad_stats_slices(geom, case.B)),
        int(X.conv_wino(geom, case.B, False)), int(X.conv_wino(geom, case.B, True)))
    assert got == case.plan, f"the bindings route this call elsewhere: {got} != {case.plan} ({R.PLAN_COLUMNS})"


# ------------------------------------------ launches -----------------------------------------
def _fwd(X, case, d, wu, defer=False, stats=False):
    """y, the split-K scratch, the statistics partials, the return value"""
    Co = case.geom[3]
    y = _nan(d["dy"].shape, d["x"].device)
    ks = case.fwd_ksplit
    part = _nan((ks * y.numel(),), y.device) if ks > 1 else None
    st = _nan((Co * case.fwd_stats_slices * 2,), y.device, torch.float64) if stats else None
    left = X.conv_fwd(d["x"], d["w"], y, list(case.geom), part, defer, st, wu)
    return y, part, st, left


def _dgrad(X, case, d, wu, addend=None, defer=False, stats=False):
    """dx, the split-K scratch (DirectConvFn._grad_x's rule: compact slabs for the 1x1 stride-2
    classes, numel(x) otherwise), the statistics partials, the return value"""
    x, dy = d["x"], d["dy"]
    C, Co = case.geom[0], case.geom[3]
    dx = _nan(x.shape, x.device)
    ks = case.dgrad_ksplit
    slab = (dy.numel() // Co) * C if case.cls in UPS else x.numel()
    part = _nan((ks * slab,), x.device) if ks > 1 else None
    st = _nan((C * case.dgrad_stats_slices * 2,), x.device, torch.float64) if stats else None
    bn = (d["bx"], d["by"], d["mean"], d["invstd"]) if stats else (None, None, None, None)
    left = X.conv_dgrad(dy, d["w"], dx, list(case.geom), part, addend, defer, st, *bn, wu)
    return dx, part, st, left


def _wgrad(X, case, d, with_dw=True, pair=False):
    """dw (None: slabs only) and the B // wgrad_imgs slabs"""
    w = d["w"]
    part = _nan(((case.B // case.wgrad_imgs) * w.numel(),), w.device)
    dw = _nan(w.shape, w.device) if with_dw else None
    X.conv_wgrad(d["x"], d["dy"], part, dw, list(case.geom), pair)
    return dw, part


# ------------------------------------------- options -----------------------------------------
def _check_forward(X, case, d, rep, wu):
    Co = case.geom[3]
    B, ks = case.B, case.fwd_ksplit
    u = wu if case.fwd_wino else None
    y, _, _, left = _fwd(X, case, d, u)
    rep.true("conv_fwd returns 1", left == 1, f"(got {left})")
    rep.close("y", y, d["ref"]["y"], case.fwd_wino)
    rep.same("y, second run", _fwd(X, case, d, u)[0], y)
    if case.fwd_wino:
        rep.same("y, wino_u built by the binding", _fwd(X, case, d, None)[0], y)
    if ks > 1:
        yd, part, _, left = _fwd(X, case, d, u, defer=True)
        rep.true("deferred conv_fwd returns fwd_ksplit", left == ks, f"(got {left}, want {ks})")
        rep.true("deferred conv_fwd leaves y unwritten", bool(torch.isnan(yd).all()))
        rep.same("forward slabs summed in order", _slab_sum(part, ks, y.numel()).view_as(y), y)
    S = case.fwd_stats_slices
    if S:
        ys, _, st, left = _fwd(X, case, d, u, stats=True)
        rep.true("conv_fwd with stats returns 1", left == 1, f"(got {left})")
        rep.same("y with the statistics epilogue", ys, y)
        OH = y.shape[2]
        if case.cls == STEM_CLS:  # one partial per (image, output-row block)
            rb = S // B
            imgs, npix = 1, OH * OH // rb
            yt = y.double().view(B, Co, rb, npix).permute(0, 2, 1, 3).reshape(S, 1, Co, npix)
        else:
            imgs, npix = B // S, OH * OH
            yt = y.double().view(S, imgs, Co, npix)
        st = st.view(Co, S, 2)
        tile_sum, tile_sq = yt.sum((1, 3)).t(), (yt * yt).sum((1, 3)).t()  # [Co][S]
        e0, e1 = (st[..., 0] - tile_sum).abs().max().item(), (st[..., 1] - tile_sq).abs().max().item()
        print(f"PLANSTAT {case.id} fwd sum err {e0:.3e} sq err {e1:.3e} tile {imgs}x{npix}")
        rep.true("forward partial sums", torch.allclose(st[..., 0], tile_sum, rtol=1e-9, atol=1e-6 * imgs * npix),
                 f"(max err {e0:.3e})")
        rep.true("forward partial squares", torch.allclose(st[..., 1], tile_sq, rtol=1e-6, atol=1e-6),
                 f"(max err {e1:.3e})")


def _check_dgrad(X, case, d, rep, wu):
    C, H = case.geom[0], case.geom[1]
    B, ks = case.B, case.dgrad_ksplit
    u = wu if case.dgrad_wino else None
    add = d["add"]
    dx, _, _, left = _dgrad(X, case, d, u)
    rep.true("conv_dgrad returns 1", left == 1, f"(got {left})")
    rep.close("dx", dx, d["ref"]["dx"], case.dgrad_wino)
    rep.same("dx, second run", _dgrad(X, case, d, u)[0], dx)
    dxa, _, _, left = _dgrad(X, case, d, u, add)
    rep.true("conv_dgrad with addend returns 1", left == 1, f"(got {left})")
    rep.close("dx+addend", dxa, d["ref"]["dx"] + add.double(), case.dgrad_wino)
    rep.same("dx + addend, second run", _dgrad(X, case, d, u, add)[0], dxa)
    if case.dgrad_wino:
        rep.same("dx, wino_u built by the binding", _dgrad(X, case, d, None)[0], dx)
    if case.cls in UPS:
        odd = torch.ones_like(dx, dtype=torch.bool)
        odd[:, :, ::2, ::2] = False
        rep.true("odd pixels of dx are zero", torch.count_nonzero(dx[odd]).item() == 0)
        rep.same("odd pixels of dx + addend are the addend", dxa[odd], add[odd])
    if ks > 1:
        dd, part, _, left = _dgrad(X, case, d, u, add, defer=True)
        if case.cls in UPS:  # the compact slabs are scattered by the launcher: it cannot defer
            rep.true("deferred 1x1 stride-2 conv_dgrad returns 1", left == 1, f"(got {left})")
            rep.same("deferred 1x1 stride-2 dx is final", dd, dxa)
        else:
            rep.true("deferred conv_dgrad returns dgrad_ksplit", left == ks, f"(got {left}, want {ks})")
            rep.true("deferred conv_dgrad leaves dx unwritten", bool(torch.isnan(dd).all()))
            rep.same("grad-x slabs summed in order", _slab_sum(part, ks, dx.numel()).view_as(dx), dx)
            rep.same("grad-x slabs summed in order, then the addend", _slab_sum(part, ks, dx.numel(), add).view_as(dx),
                     dxa)
    S = case.dgrad_stats_slices
    if S:
        mask = (d["by"] > 0).double()
        xh = (d["bx"].double() - d["mean"].double().view(1, C, 1, 1)) * d["invstd"].double().view(1, C, 1, 1)
        for name, addend, plain in (("", None, dx), ("+addend", add, dxa)):
            ds, _, st, left = _dgrad(X, case, d, u, addend, stats=True)
            rep.true(f"conv_dgrad{name} with stats returns 1", left == 1, f"(got {left})")
            rep.same(f"dx{name} with the statistics epilogue", ds, plain)
            dz = plain.double() * mask  # dz from dx including the addend
            ref_a = dz.sum((2, 3)).view(S, B // S, C).sum(1).t()
            ref_b = (dz * xh).sum((2, 3)).view(S, B // S, C).sum(1).t()
            st = st.view(C, S, 2)
            tol = 1e-5 * (dz.abs().max().item() * H * H)
            ea, eb = (st[..., 0] - ref_a).abs().max().item(), (st[..., 1] - ref_b).abs().max().item()
            print(f"PLANSTAT {case.id} dgrad{name} sum err {ea:.3e} (tol {tol:.3e}) xhat err {eb:.3e} "
                  f"(tol {8 * tol:.3e}) tile {B // S}")
            rep.true(f"grad-x{name} partial sums of dz", ea < tol, f"(err {ea:.3e}, tol {tol:.3e})")
            rep.true(f"grad-x{name} partial sums of dz * xhat", eb < 8 * tol, f"(err {eb:.3e}, tol {8 * tol:.3e})")
    return dx, dxa


def _check_wgrad(X, case, d, rep):
    wino = case.cls == 0 and bool(case.wino)  # launch_conv_wgrad reads the switch, not the plan
    n, numel = case.B // case.wgrad_imgs, d["w"].numel()
    dw, part = _wgrad(X, case, d)
    rep.close("dw", dw, d["ref"]["dw"], wino)
    rep.same("dw, second run", _wgrad(X, case, d)[0], dw)
    rep.same("grad-W slabs of the summed launch, summed in order", _slab_sum(part, n, numel).view_as(dw), dw)
    none, part = _wgrad(X, case, d, with_dw=False)
    assert none is None
    rep.same("grad-W slabs (dw=None) summed in order", _slab_sum(part, n, numel).view_as(dw), dw)
    return dw


def _pairs(case):
    """does a held-back grad-W run in the grad-x launch (module docstring)"""
    if case.cls in UPS:
        return True
    return bool(case.dgrad_wino) and (case.cls in (0, 1) or (case.cls == 2 and case.B <= 256))


def _check_pair(X, case, d, rep, wu, dx, dxa, dw):
    n, numel = case.B // case.wgrad_imgs, d["w"].numel()
    u = wu if case.dgrad_wino else None
    for name, addend, plain in (("", None, dx), ("+addend", d["add"], dxa)):
        before = X.conv_pair_launches()
        _, part = _wgrad(X, case, d, with_dw=False, pair=True)
        got = None
        if case.dgrad_direct:
            got, _, _, left = _dgrad(X, case, d, u, addend)
            rep.true(f"paired conv_dgrad{name} returns 1", left == 1, f"(got {left})")
        count = X.conv_pair_launches() - before
        X.conv_flush_pending()
        want = 1 if (case.dgrad_direct and _pairs(case)) else 0
        rep.true(f"pair launches{name}", count == want, f"(got {count}, want {want})")
        rep.true(f"flush launches no pair{name}", X.conv_pair_launches() - before == count)
        if got is not None:
            rep.same(f"paired dx{name}", got, plain)
        rep.same(f"paired grad-W slabs{name} summed in order", _slab_sum(part, n, numel).view_as(dw), dw)
        if not case.dgrad_direct:
            break  # the stem: no grad-x, one round


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_conv_plan_case_vs_fp64(device, case):
    from network_distributed_pytorch_amd.ops._ext import ext
    from network_distributed_pytorch_amd.ops.conv import set_winograd

    X = ext()
    d = _data(case, device)
    rep = _Report(case)
    try:
        set_winograd(bool(case.wino))
        X.conv_set_stem_psplit(case.psplit)
        _assert_plan(X, case)
        wu = None
        if case.fwd_wino or case.dgrad_wino:  # forward + grad-x layouts, built once and shared
            wu = torch.empty(32 * d["w"].numel() // 9, device=device)
            X.wino_weights(d["w"], wu)
        _check_forward(X, case, d, rep, wu)
        dx = dxa = None
        if case.dgrad_direct:
            dx, dxa = _check_dgrad(X, case, d, rep, wu)
        dw = _check_wgrad(X, case, d, rep)
        _check_pair(X, case, d, rep, wu, dx, dxa, dw)
    finally:
        X.conv_flush_pending()  # nothing held leaks into the next test
        X.conv_set_stem_psplit(0)
        set_winograd(True)
    for k, v in d["host"].items():
        rep.same(f"input {k} unmodified", d[k].cpu(), v)
    assert not rep.bad, f"{case.id}: " + "; ".join(rep.bad)
