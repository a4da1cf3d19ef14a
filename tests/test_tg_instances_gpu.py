"""Every reachable tgemm kernel instance (csrc/tgemm.hip), one launch per Case of tests/tg_cases.py,
through the bindings tg_fwd / tg_dgrad / tg_wgrad so that the scratch, defer, the addend and the
operand alignment are the test's own.

Per case, before anything is launched, tg_describe with the operands' real data_ptr() % 16 must name
the case's instance and slab count (it shares that decision with the launch).  Then

  * integer operands in [-3, 3]: every product and every partial sum is an integer below 2^24
    (9 K <= 9504), so fp32 accumulates exactly in any order and the result must be torch.equal to
    the fp64 conv2d / conv2d_input / conv2d_weight reference cast to fp32 -- through split-K and the
    slab sum, plus the addend; each split-K slab must equal the reference restricted to its k range
    [z kchunk, min(K, (z + 1) kchunk));
  * randn operands: max abs error / max |ref| < 2e-5 against fp64, the bound of
    tests/test_tgconv_gpu.py; each comparison prints "TGERR <case> <dir> <instance> err scale"
    before it is judged (worst err / scale seen on an MI355X: 3.9e-7 forward, 3.1e-7 grad-x,
    3.5e-7 grad-W);
  * outputs and scratch sit inside larger buffers between 64-float guard bands (so the payload stays
    16-byte aligned), outputs pre-filled with NaN: afterwards no NaN in what the launch owns, guards
    untouched, scratch slabs past the launched count untouched, and under defer the output untouched
    and the returned count equal to tg_describe's;
  * a second run is bitwise equal.

Misalignment (4 bytes) is applied to read-only operands alone, where the dispatcher falls back to
4-byte loads; a misaligned output of a launch that sums slabs is refused by the bindings before any
launch, which is all that is tested of it.
"""
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

from network_distributed_pytorch_amd.ops import ext
from network_distributed_pytorch_amd.ops.tgconv import POINTWISE, TgConvFn, tg_plan
from tests import tg_cases as T

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -12345.0
NAN = float("nan")
BOUND = 2e-5


def _bits(t):
    return t.view(torch.int32)


def _offset_copy(t, off_bytes, device):
    """a contiguous device copy of ``t`` whose base sits ``off_bytes`` past a 16-byte boundary"""
    n, k = t.numel(), off_bytes // 4
    buf = torch.zeros(n + 4, device=device)
    assert buf.data_ptr() % 16 == 0
    v = buf[k:k + n].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == off_bytes
    return v


class Guarded:
    """``shape`` floats between two guard bands of one buffer"""

    def __init__(self, shape, device, fill):
        self.n = math.prod(shape)
        self.buf = torch.full((self.n + 2 * GUARD,), SENTINEL, device=device)
        assert self.buf.data_ptr() % 16 == 0
        self.t = self.buf[GUARD:GUARD + self.n].view(shape)
        if isinstance(fill, torch.Tensor):
            self.t.copy_(fill)
        else:
            self.t.fill_(fill)
        self.before = self.buf.clone()

    def guards_intact(self):
        g = torch.cat([self.buf[:GUARD], self.buf[GUARD + self.n:]])
        return bool((_bits(g) == _bits(torch.tensor([SENTINEL], device=g.device))).all())

    def untouched(self, lo=0, hi=None):
        """payload elements [lo, hi) hold the bits they were filled with"""
        a = self.buf[GUARD + lo:GUARD + (self.n if hi is None else hi)]
        b = self.before[GUARD + lo:GUARD + (self.n if hi is None else hi)]
        return torch.equal(_bits(a), _bits(b))


def _operands(case, kind):
    """x, w, dy, addend on the CPU, fp32"""
    B, C, H, W, Co = case.shape
    g = torch.Generator().manual_seed(zlib.crc32(f"{case.name}/{kind}".encode()))

    def draw(*shape):
        if kind == "int":
            return torch.randint(-3, 4, shape, generator=g).float()
        return torch.randn(shape, generator=g)

    return draw(B, C, H, W), draw(Co, C, 1, 1), draw(B, Co, H, W), draw(B, C, H, W)


def _reference(case, x, w, dy, k0=0, k1=None):
    """the fp64 result of the case's direction with the reduction restricted to k in [k0, k1)"""
    B, C, H, W, Co = case.shape
    x, w, dy = x.double(), w.double(), dy.double()
    k1 = case.K if k1 is None else k1
    if case.dir == T.FWD:      # k = c
        xs = torch.zeros_like(x)
        xs[:, k0:k1] = x[:, k0:k1]
        return F.conv2d(xs, w)
    if case.dir == T.DGRAD:    # k = co
        ds = torch.zeros_like(dy)
        ds[:, k0:k1] = dy[:, k0:k1]
        return torch.nn.grad.conv2d_input(x.shape, w, ds)
    k = torch.arange(B * H * W).view(B, 1, H, W)   # k = (image, pixel)
    return torch.nn.grad.conv2d_weight(x, w.shape, dy * ((k >= k0) & (k < k1)))


class Run:
    """one launch of a case: operands placed, instance asserted, launched, results on the CPU"""

    def __init__(self, case, device, x, w, dy, addend):
        B, C, H, W, Co = case.shape
        e = ext()
        if case.dir == T.FWD:
            a, b = _offset_copy(w, case.a_off, device), _offset_copy(x, case.b_off, device)
            oshape = (B, Co, H, W)
        elif case.dir == T.DGRAD:
            a, b = _offset_copy(w, case.a_off, device), _offset_copy(dy, case.b_off, device)
            oshape = (B, C, H, W)
        else:
            a, b = _offset_copy(dy, case.a_off, device), _offset_copy(x, case.b_off, device)
            oshape = (Co, C, 1, 1)
        d = e.tg_describe(case.geom, B, case.dir, a.data_ptr() % 16, b.data_ptr() % 16)
        assert T.instance_name(d) == case.instance, (case.name, d)
        assert (d["M"], d["N"], d["K"]) == (case.M, case.N, case.K)
        assert (d["splits"], d["slabs"], d["kchunk"]) == (case.splits, case.slabs, case.kchunk)
        self.slab = d["slab"]
        assert self.slab == math.prod(oshape)
        self.out = Guarded(oshape, device, addend if case.addend else NAN)
        self.part = Guarded((case.splits * self.slab,), device, NAN) if case.splits > 1 else None
        p = self.part.t if self.part is not None else None
        if case.dir == T.FWD:
            self.left = e.tg_fwd(b, a, self.out.t, case.geom, p, case.defer)
        elif case.dir == T.DGRAD:
            self.left = e.tg_dgrad(b, a, self.out.t, case.geom, p, self.out.t if case.addend else None, case.defer)
        else:
            self.left = e.tg_wgrad(b, a, self.out.t, case.geom, p, case.defer)
        torch.cuda.synchronize()
        self.result = self.out.t.cpu()
        self.slabs = self.part.t.cpu().view(case.splits, *oshape) if self.part is not None else None


def _err(case, what, got, ref):
    scale = ref.abs().max().item()
    err = (got.double() - ref).abs().max().item()
    print(f"TGERR {case.name}{what} {T.DIR_NAMES[case.dir]} {case.instance} err {err:.3e} scale {scale:.3e}")
    return err / (scale + 1e-30)


def _check(case, device, kind):
    x, w, dy, addend = _operands(case, kind)
    r = Run(case, device, x, w, dy, addend)
    bad = []
    deferred = case.defer and case.slabs > 1
    if r.left != (case.slabs if deferred else 1):
        bad.append(f"returned {r.left} slabs, tg_describe says {case.slabs}")
    # nothing outside, nothing unwritten
    if not r.out.guards_intact():
        bad.append("output guard band written")
    if deferred:
        if not r.out.untouched():
            bad.append("deferred launch wrote the output")
    elif torch.isnan(r.result).any():
        bad.append(f"{int(torch.isnan(r.result).sum())} output elements unwritten")
    if r.part is not None:
        if not r.part.guards_intact():
            bad.append("scratch guard band written")
        if not r.part.untouched(case.slabs * r.slab):
            bad.append("scratch written past the launched slabs")
        if case.slabs > 1 and torch.isnan(r.slabs[:case.slabs]).any():
            bad.append("scratch slab elements unwritten")
        if case.slabs == 1 and not r.part.untouched():
            bad.append("single-split launch wrote the scratch")
    # values
    ref = _reference(case, x, w, dy)
    total = ref + addend.double() if case.addend else ref
    if kind == "int":
        if not deferred and not torch.equal(r.result, total.float()):
            bad.append(f"output: {int((r.result != total.float()).sum())} of {total.numel()} elements differ")
        if case.slabs > 1:
            for z in range(case.slabs):
                rz = _reference(case, x, w, dy, z * case.kchunk, min(case.K, (z + 1) * case.kchunk)).float()
                if not torch.equal(r.slabs[z], rz):
                    bad.append(f"slab {z}: {int((r.slabs[z] != rz).sum())} of {rz.numel()} elements differ")
    else:
        if not deferred:
            e = _err(case, "", r.result, total)
            if not e < BOUND:
                bad.append(f"output: rel err {e:.3g}")
        if case.slabs > 1:
            e = _err(case, "/slabs", r.slabs[:case.slabs].double().sum(0), ref)
            if not e < BOUND:
                bad.append(f"slab sum: rel err {e:.3g}")
    # determinism
    r2 = Run(case, device, x, w, dy, addend)
    if r2.left != r.left or not torch.equal(_bits(r2.out.buf), _bits(r.out.buf)):
        bad.append("second run differs in the output")
    if r.part is not None and not torch.equal(_bits(r2.part.buf), _bits(r.part.buf)):
        bad.append("second run differs in the scratch")
    assert not bad, f"{case.name} {kind} {case.instance}: " + "; ".join(bad)


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_tg_instance_exact_on_integers(device, case):
    _check(case, device, "int")


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_tg_instance_rounding(device, case):
    _check(case, device, "randn")


@pytest.mark.parametrize("name", ["fwd-m68-split2", "dgrad-m68-split2", "wgrad-m72-split2"])
def test_misaligned_output_of_a_slab_sum_is_refused(device, name):
    """conv_slab_sum stores float4: tg_fwd / tg_dgrad / tg_wgrad raise before any launch"""
    case = T.by_name(name)
    B, C, H, W, Co = case.shape
    assert case.slabs > 1 and not case.defer
    x, w, dy = (torch.zeros(s, device=device) for s in ((B, C, H, W), (Co, C, 1, 1), (B, Co, H, W)))
    oshape = [(B, Co, H, W), (B, C, H, W), (Co, C, 1, 1)][case.dir]
    out = _offset_copy(torch.full(oshape, NAN), 4, device)
    part = Guarded((case.splits * out.numel(),), device, NAN)
    with pytest.raises(RuntimeError, match="16-B aligned"):
        if case.dir == T.FWD:
            ext().tg_fwd(x, w, out, case.geom, part.t, False)
        elif case.dir == T.DGRAD:
            ext().tg_dgrad(dy, w, out, case.geom, part.t, None, False)
        else:
            ext().tg_wgrad(x, dy, out, case.geom, part.t, False)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and part.untouched() and part.guards_intact()


@pytest.mark.parametrize("shape,fwd,dgrad,wgrad", [
    ((4, 18, 4, 4, 20), "TT14", "FT14", "TF44"),    # C % 4 != 0: scalar weight loads at any alignment
    ((6, 36, 4, 4, 40), "TT14", "FT14", "TF44"),    # C % 4 == 0: scalar weight loads by the offset alone
])
def test_tgconv_autograd_reaches_scalar_instances(device, shape, fwd, dgrad, wgrad):
    """the public path (TgConvFn) with a weight viewed 4 bytes into a larger buffer: the scalar-load
    instances run and match fp64"""
    B, C, H, W, Co = shape
    g = torch.Generator().manual_seed(zlib.crc32(repr(shape).encode()))
    x0, w0, dy0 = torch.randn(B, C, H, W, generator=g), torch.randn(Co, C, 1, 1, generator=g), \
        torch.randn(B, Co, H, W, generator=g)
    x = x0.to(device).requires_grad_()
    wv = _offset_copy(w0, 4, device).requires_grad_()
    dy = dy0.to(device)
    plan = tg_plan(x, wv, 1, 0)
    assert plan is not None and plan[1] == POINTWISE
    geom = list(plan[0])
    al = lambda t: t.data_ptr() % 16  # noqa: E731
    inst = [T.instance_name(ext().tg_describe(geom, B, d, al(a), al(b)))
            for d, a, b in ((T.FWD, wv, x), (T.DGRAD, wv, dy), (T.WGRAD, dy, x))]
    assert inst == [fwd, dgrad, wgrad]
    y = TgConvFn.apply(x, wv, plan)
    y.backward(dy)
    xr, wr = x0.double().requires_grad_(), w0.double().requires_grad_()
    yr = F.conv2d(xr, wr)
    yr.backward(dy0.double())
    for what, got, ref in (("fwd", y, yr), ("dgrad", x.grad, xr.grad), ("wgrad", wv.grad, wr.grad)):
        scale = ref.abs().max().item()
        err = (got.detach().double().cpu() - ref.detach()).abs().max().item()
        print(f"TGERR autograd-{C}x{H}x{W}-{Co} {what} {dict(fwd=fwd, dgrad=dgrad, wgrad=wgrad)[what]} "
              f"err {err:.3e} scale {scale:.3e}")
        assert err / scale < BOUND, (what, err, scale)
