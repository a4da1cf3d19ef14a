"""Every BatchNorm launch variant of csrc/batchnorm.hip against an fp64 oracle, through the bindings.

tests/bn_route_cases.py lists one call per variant key (binding, mode, map size, route row of the
recorded table); tests/test_bn_route_cases_cpu.py pins that the list leaves no key out.  Each case
here builds the call's operands (slab tensors, the grad-x addend, conv-epilogue partials, operands
one float past a 16-byte boundary), asks bn_route what those very tensors would launch, asserts
that this is the case's route row, launches, and compares every tensor the binding writes with
plain fp64 torch written out below.  So a wrong instantiation fails, and the premise proves that
it was reached.

The ReLU mask never decides a verdict: the inputs are conditioned on the CPU until every fp64
pre-activation is at least MARGIN from zero (about 100 times the worst fp32 rounding of
fma(x, scale, shift) at these magnitudes, 8 * 2^-23 ~ 1e-6), the device mask is then asserted equal
to the fp64 mask, and the backward oracle uses that mask.  Each case runs twice from identical
inputs and every output must be bitwise equal.

Alignment: a `False` of the call's align tuple becomes a real operand one float past a 16-byte
boundary.  bn_fwd / bn_bwd operands belong to the single-launch set and the two-kernel set at
once, so the fact that the case's path reads decides (the other is whatever the tensors give);
the premise is asserted on the facts of the tensors as built.

bn_fwd / bn_bwd keys run the three (residual, relu) arms of tools/bn_route_sweep.py; a key with the
mask recomputed from x (mbeta) has the one arm that the bindings define for it (relu, no residual).
The keys bn_bwd-mbeta-HW*-r55 (mbeta with an operand off a 16-byte boundary: the scalar two-kernel
backward) are the regression test for a read of the absent y through a null pointer there.
"""
import zlib

import pytest
import torch
import torch.nn.functional as F

from tests import bn_route_cases as R
from tools import bn_route_table as T

pytestmark = pytest.mark.gpu

EPS, MOM, MARGIN = 1e-5, 0.1, 1e-4
ARMS = ((False, True), (True, True), (False, False))  # (residual, relu), as tools/bn_route_sweep.py
PARTIAL = ("path", "v4", "CW", "split", "vec", "slab", "addend")  # asserted on the relu = False arm
FUSED = (1, 2)  # paths that read the single-launch alignment fact
NAN = float("nan")


# ----------------------------------------- operands ------------------------------------------
class _Rng:
    """seeded on the CPU from the case id"""

    def __init__(self, tag):
        self.gen = torch.Generator().manual_seed(zlib.crc32(tag.encode()))

    def __call__(self, *shape, scale=1.0, bias=0.0):
        return torch.randn(*shape, generator=self.gen) * scale + bias


class _Params:
    """gamma, beta and the running statistics of tools/bn_route_sweep.py Sweep.params"""

    def __init__(self, rng, C):
        self.gamma, self.beta = rng(C, scale=0.3, bias=1.0), rng(C, scale=0.3)
        self.rmean, self.rvar = rng(C, scale=0.1), rng(C, scale=0.05, bias=1.0).abs()

    def dev(self, dev):
        C = self.gamma.numel()
        return dict(gamma=_put(self.gamma, dev), beta=_put(self.beta, dev), rmean=_put(self.rmean, dev),
                    rvar=_put(self.rvar, dev), nbt=torch.zeros(1, dtype=torch.int64, device=dev),
                    sm=_put(torch.full((C,), NAN), dev), si=_put(torch.full((C,), NAN), dev))


def _put(t, dev, shift=False):
    """t on the device: 16-byte aligned, or (shift) a contiguous view one float past such a boundary"""
    buf = torch.empty(t.numel() + (1 if shift else 0), dtype=t.dtype, device=dev)
    v = buf[1:] if shift else buf
    v = v.view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 if shift else 0) and v.is_contiguous()
    return v


def _nan(shape, dev, shift=False):
    """an output: every element must be written"""
    return _put(torch.full(tuple(shape), NAN), dev, shift)


def _a16(*ts):
    return all(t is None or t.data_ptr() % 16 == 0 for t in ts)


def _pick(case, names):
    """the operand of the set that is misaligned in this case: a different one from case to case"""
    return names[zlib.crc32(case.id.encode()) % len(names)]


def _misaligned(case):
    """does the alignment fact that the case's path reads ask for a misaligned operand?"""
    fused, two, _slabs, _slabs2 = case.align
    return not (fused if case.path in FUSED else two)


def _slabs(rng, t, n):
    """n stacked slabs whose sum is t up to rounding (n = 1: one slab of noise, which the bindings
    ignore); None for n = 0"""
    if n < 1:
        return None
    if n == 1:
        return rng(*t.shape, scale=0.6).unsqueeze(0).contiguous()
    rest = [rng(*t.shape, scale=0.6) for _ in range(n - 1)]
    return torch.stack([t - sum(rest)] + rest).contiguous()


def _seqsum(slabs, addend=None):
    """the fp32 sum in slab order, the addend last: what the launch is expected to write"""
    s = slabs[0].clone()
    for z in range(1, slabs.shape[0]):
        s += slabs[z]
    return s if addend is None else s + addend


def _ext_stats(a, b, slices):
    """[C][slices][2] fp64 sums of a and a * b over `slices` contiguous groups of images, as a conv
    epilogue emits them (tools/bn_route_sweep.py Sweep.image_stats, grouped)"""
    N, C = a.shape[:2]
    per = torch.stack([a.reshape(N, C, -1).sum(2), (a * b).reshape(N, C, -1).sum(2)], dim=2)  # [N][C][2]
    groups = torch.tensor_split(torch.arange(N), slices)
    return torch.stack([per[g].sum(0) for g in groups]).permute(1, 0, 2).contiguous()


# ------------------------------------------ oracle -------------------------------------------
def _v(t):
    return t.double().view(1, -1, 1, 1)


def _batch_stats(xd):
    """biased mean and variance over N * HW, fp64, shaped [1, C, 1, 1]"""
    mean = xd.mean((0, 2, 3), keepdim=True)
    return mean, ((xd - mean) ** 2).mean((0, 2, 3), keepdim=True)


def _bn(xd, p, mean, var):
    return _v(p.gamma) * (xd - mean) * (var + EPS).rsqrt() + _v(p.beta)


def _bn_bwd(dz, xd, p, mean, var):
    """the standard BN gradients of z = gamma * xhat + beta for a given dz: dx, dgamma, dbeta"""
    M = xd.numel() // xd.shape[1]
    invstd = (var + EPS).rsqrt()
    xhat = (xd - mean) * invstd
    dbeta, dgamma = dz.sum((0, 2, 3), keepdim=True), (dz * xhat).sum((0, 2, 3), keepdim=True)
    dx = _v(p.gamma) * invstd * (dz - dbeta / M - xhat * dgamma / M)
    return dx, dgamma.flatten(), dbeta.flatten()


def _condition(z_of, nudged, sign=None, extra=None):
    """Move inputs until no fp64 pre-activation z_of() lies inside (-MARGIN, MARGIN): elements inside
    get nudged += 1e-2 * sign(z + tiny).  extra(z) -> mask of further elements to raise (the stem's
    window ties), looked at once the margin holds.  A condition on the inputs, established by the
    reference alone; it must converge within 8 passes."""
    for _ in range(8):
        z = z_of()
        bad = z.abs() < MARGIN
        if bad.any():
            nudged[bad] += (1e-2 * torch.sign(z[bad] + 1e-300)).float()
            continue
        more = extra(z) if extra is not None else None
        if more is None or not more.any():
            return
        nudged += 1e-2 * more.float() * sign
    z = z_of()
    assert not (z.abs() < MARGIN).any() and (extra is None or not extra(z).any()), "conditioning did not converge"


def _close(got, ref, tol, what):
    """tests/test_bn_pair_gpu.py _close: relative to the reference's largest magnitude"""
    err = (got.double() - ref.double()).abs().max().item()
    scale = ref.abs().max().item() + 1e-12
    assert err <= tol * scale + 1e-7, (what, err, scale)  # (nan fails)


def _near(got, ref, what, rtol, atol):
    print(f"{what}: max abs err {(got.double() - ref).abs().max().item():.3e}")
    torch.testing.assert_close(got.double(), ref, rtol=rtol, atol=atol, msg=lambda m: f"{what}: {m}")


def _check_sum(got, slabs, addend, what):
    """the tensor the launch wrote = the fp64 sum of the slabs (+ addend), within nslab roundings"""
    n = slabs.shape[0]
    terms = slabs.double() if addend is None else torch.cat([slabs.double(), addend.double().unsqueeze(0)])
    err = (got.double() - terms.sum(0)).abs()
    bound = n * 2.0 ** -24 * terms.abs().sum(0)
    assert bool((err <= bound).all()), (what, err.max().item())


def _summed_dy(case, got, slabs, addend):
    """The backward's fp64 input gradient.  A launch that sums slabs writes dy, and the oracle goes on
    from that device-written tensor once it is checked against the fp64 sum (a wrong sum and a wrong
    BN fail apart) -- except the single-launch backward with the slabs summed in the kernel: it keeps
    the sum in registers and leaves dy alone (nothing reads dy after a BN backward), so there the
    oracle takes the fp64 sum itself."""
    if slabs is None or slabs.shape[0] < 2:
        return got.double()
    if case.path in FUSED and case.slab == 1:
        return slabs.double().sum(0) + (addend.double() if addend is not None else 0.0)
    _check_sum(got, slabs, addend, "summed dy")
    return got.double()


def _check_fwd_stats(o, p, mean, var, M, sfx=""):
    unb = var * M / (M - 1)
    _close(o["save_mean" + sfx], mean.flatten(), 1e-6, "save_mean" + sfx)
    _close(o["save_invstd" + sfx], (var + EPS).rsqrt().flatten(), 1e-6, "save_invstd" + sfx)
    _close(o["running_mean" + sfx], (1 - MOM) * p.rmean.double() + MOM * mean.flatten(), 1e-6, "running_mean" + sfx)
    _close(o["running_var" + sfx], (1 - MOM) * p.rvar.double() + MOM * unb.flatten(), 1e-6, "running_var" + sfx)
    assert o["num_batches_tracked" + sfx].item() == 1


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _twice(launch):
    """both runs' outputs bitwise equal; the first run's outputs"""
    a, b = launch(), launch()
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), f"{k} differs between two runs from identical inputs"
    return a


def _cpu(**tensors):
    return {k: v.detach().cpu().clone() for k, v in tensors.items() if v is not None}


# ------------------------------------------ premise ------------------------------------------
def _premise(X, case, align, relu=True, full=True):
    """bn_route on the facts of the tensors as built sends the call down the case's route"""
    c = dict(zip(T.CALL_COLUMNS, case.call))
    got = X.bn_route(bool(c["bwd"]), case.N, case.C, case.HW, training=bool(c["training"]), single=bool(c["single"]),
                     pair=bool(c["pair"]), pool_w=c["pool_w"], nslab=c["nslab"], nslab2=c["nslab2"],
                     ext_slices=c["ext_slices"], relu=relu, addend=bool(c["addend"]), mbeta=bool(c["mbeta"]),
                     align=[bool(a) for a in align])
    r = dict(zip(T.ROUTE_COLUMNS, (int(v) for v in got)))
    want = dict(zip(T.COLUMNS, case.route))
    cols = T.COLUMNS if full else PARTIAL
    assert {k: r[k] for k in cols} == {k: want[k] for k in cols}, (case.id, align)
    S, Sa, Ss, part_numel, blocks = case.shape
    assert (r["S"], r["Sa"], r["Ss"], r["part_numel"]) == (S, Sa, Ss, part_numel)
    assert r["grid"] == (blocks * r["split"] if r["path"] in FUSED else 0)
    return r


def _part(r, dev):
    return torch.zeros(r["part_numel"], dtype=torch.float64, device=dev)


# ------------------------------------------- bn_fwd ------------------------------------------
def _check_bn_fwd(X, dev, case, res, relu):
    N, C, HW, ns, training = case.N, case.C, case.HW, case.nslab, bool(case.training)
    shape = (N, C, HW, 1)
    rng = _Rng(f"{case.id}/res{int(res)}relu{int(relu)}")
    p = _Params(rng, C)
    x = rng(*shape, scale=1.7, bias=0.4)
    r = rng(*shape) if res else None
    slabs = _slabs(rng, x, ns)
    summed = ns >= 2

    def stats(xd):
        return _batch_stats(xd) if training else (_v(p.rmean), _v(p.rvar))

    def z_of(xin=None):
        xd = (xin if xin is not None else _seqsum(slabs) if summed else x).double()
        return _bn(xd, p, *stats(xd)) + (r.double() if res else 0.0)

    if relu:
        _condition(z_of, r if res else slabs[0] if summed else x)
    xst = _ext_stats(x.double(), x.double(), case.ext_slices) if case.ext_slices else None
    shifted = {_pick(case, ["x", "y"] + (["res"] if res else []))} if _misaligned(case) else set()

    def launch():
        d = p.dev(dev)
        xin = _nan(shape, dev, "x" in shifted) if summed else _put(x, dev, "x" in shifted)
        rin = _put(r, dev, "res" in shifted) if res else None
        y = _nan(shape, dev, "y" in shifted)
        xpart = _put(slabs, dev, not case.align[2]) if slabs is not None else None
        st = _put(xst, dev) if xst is not None else None
        al = (_a16(xin, rin, y), _a16(xin, rin, y), _a16(xpart if summed else None), True)
        route = _premise(X, case, al, relu=relu, full=relu)
        X.bn_fwd(xin, rin, y, d["gamma"], d["beta"], d["rmean"], d["rvar"], d["nbt"], d["sm"], d["si"],
                 _part(route, dev), EPS, MOM, relu, training, bool(case.single), xpart, ns, st,
                 case.ext_slices if st is not None else 0)
        return _cpu(y=y, x=xin, save_mean=d["sm"], save_invstd=d["si"], running_mean=d["rmean"],
                    running_var=d["rvar"], num_batches_tracked=d["nbt"])

    o = _twice(launch)
    if summed:
        _check_sum(o["x"], slabs, None, "summed x")
    xd = o["x"].double()
    mean, var = stats(xd)
    z = z_of(o["x"])
    if relu:
        assert torch.equal(o["y"] > 0, z > 0), "the device ReLU mask differs from the fp64 mask"
    _near(o["y"], torch.relu(z) if relu else z, "y", 1e-5, 2e-5)
    if training:
        _check_fwd_stats(o, p, mean, var, N * HW)
    else:  # evaluation mode: the running statistics stay bitwise untouched
        assert torch.equal(_bits(o["running_mean"]), _bits(p.rmean)) and torch.equal(_bits(o["running_var"]), _bits(p.rvar))
        assert o["num_batches_tracked"].item() == 0


# ------------------------------------------- bn_bwd ------------------------------------------
def _check_bn_bwd(X, dev, case, res, relu):
    N, C, HW, ns = case.N, case.C, case.HW, case.nslab
    mbeta, addend = bool(case.mbeta), bool(case.addend)
    shape = (N, C, HW, 1)
    rng = _Rng(f"{case.id}/res{int(res)}relu{int(relu)}")
    p = _Params(rng, C)
    x = rng(*shape, scale=1.7, bias=0.4)
    r = rng(*shape) if res else None

    def z_of():
        xd = x.double()
        return _bn(xd, p, *_batch_stats(xd)) + (r.double() if res else 0.0)

    if relu:
        _condition(z_of, r if res else x)
    xd = x.double()
    mean, var = _batch_stats(xd)
    z = z_of()
    mask = (z > 0) if relu else torch.ones_like(z, dtype=torch.bool)
    dy = rng(*shape)
    slabs = _slabs(rng, dy, ns)
    summed = ns >= 2
    dyadd = rng(*shape) if addend else None
    names = ["x", "dy", "dx"] + (["y"] if relu and not mbeta else []) + (["dres"] if res else [])
    shifted = {_pick(case, names)} if _misaligned(case) else set()
    if not case.align[2]:
        shifted.add(_pick(case, ["slabs"] + (["dyadd"] if addend else [])))

    def launch():
        # the forward that a backward follows: plain, aligned, the same (residual, relu)
        d = p.dev(dev)
        xa, ra, y = _put(x, dev), (_put(r, dev) if res else None), _nan(shape, dev)
        part = torch.zeros(int(X.bn_part_numel(N, C, HW)), dtype=torch.float64, device=dev)
        X.bn_fwd(xa, ra, y, d["gamma"], d["beta"], d["rmean"], d["rvar"], d["nbt"], d["sm"], d["si"], part, EPS, MOM,
                 relu, True, bool(case.single))
        sm, si = d["sm"].cpu(), d["si"].cpu()
        if mbeta:  # the mask as the kernels recompute it from x, in fp32
            sc = p.gamma * si
            dmask = torch.addcmul((p.beta - sm * sc).view(1, C, 1, 1), x, sc.view(1, C, 1, 1)) > 0
        else:
            dmask = y.cpu() > 0
        if relu:
            assert torch.equal(dmask, mask), "the device ReLU mask differs from the fp64 mask"
        dst = None
        if case.ext_slices:  # sums of dz and dz * xhat from the fp32 inputs, in fp64
            xh = (x.double() - _v(sm)) * _v(si)
            dst = _put(_ext_stats(dy.double() * mask, xh, case.ext_slices), dev)
        xin = _put(x, dev, "x" in shifted)
        yin = _put(y.cpu(), dev, "y" in shifted) if relu and not mbeta else None
        dyin = _nan(shape, dev, "dy" in shifted) if summed else _put(dy, dev, "dy" in shifted)
        dypart = _put(slabs, dev, "slabs" in shifted) if slabs is not None else None
        add = _put(dyadd, dev, "dyadd" in shifted) if addend else None
        dx = _nan(shape, dev, "dx" in shifted)
        dres = _nan(shape, dev, "dres" in shifted) if res else None
        dg, db = _nan((C,), dev), _nan((C,), dev)
        al = (_a16(xin, dyin, yin, dx, dres), _a16(dyin, xin, dx, yin, dres), _a16(dypart if summed else None, add), True)
        route = _premise(X, case, al, relu=relu, full=relu)
        X.bn_bwd(dyin, yin, xin, d["gamma"], d["sm"], d["si"], dx, dres, dg, db, _part(route, dev), relu,
                 bool(case.single), dypart, ns, add, d["beta"] if mbeta else None, dst,
                 case.ext_slices if dst is not None else 0)
        return _cpu(dx=dx, dres=dres, dgamma=dg, dbeta=db, dy=dyin, y=y, save_mean=d["sm"], save_invstd=d["si"])

    o = _twice(launch)
    dz = _summed_dy(case, o["dy"], slabs, dyadd) * mask
    dx, dgamma, dbeta = _bn_bwd(dz, xd, p, mean, var)
    _near(o["dx"], dx, "dx", 1e-4, 5e-5)
    _near(o["dgamma"], dgamma, "dgamma", 1e-5, 1e-4)
    _near(o["dbeta"], dbeta, "dbeta", 1e-5, 1e-4)
    if res:
        _near(o["dres"], dz, "dres", 0.0, 1e-6)


# ------------------------------------------ the pair -----------------------------------------
def _pair_inputs(case, rng):
    shape = (case.N, case.C, case.HW, 1)
    return shape, _Params(rng, case.C), _Params(rng, case.C), rng(*shape, scale=1.3, bias=0.2), \
        rng(*shape, scale=0.7, bias=-0.1)


def _pair_fwd_call(X, d, d2, x, x2, y, xpart=None, ns=0, x2part=None, ns2=0):
    X.bn_pair_fwd(x, x2, y, d["gamma"], d["beta"], d["rmean"], d["rvar"], d["nbt"], d["sm"], d["si"], d2["gamma"],
                  d2["beta"], d2["rmean"], d2["rvar"], d2["nbt"], d2["sm"], d2["si"], EPS, MOM, xpart, ns, x2part, ns2)


def _check_pair_fwd(X, dev, case):
    N, HW, ns, ns2 = case.N, case.HW, case.nslab, case.nslab2
    shape, p, p2, x, x2 = _pair_inputs(case, _Rng(case.id))
    rng = _Rng(case.id + "/slabs")
    slabs, slabs2 = _slabs(rng, x, ns), _slabs(rng, x2, ns2)
    summed, summed2 = ns >= 2, ns2 >= 2
    x2v = _seqsum(slabs2) if summed2 else x2

    def z_of(xin=None, x2in=None):
        xd = (xin if xin is not None else _seqsum(slabs) if summed else x).double()
        x2d = (x2in if x2in is not None else x2v).double()
        return _bn(xd, p, *_batch_stats(xd)) + _bn(x2d, p2, *_batch_stats(x2d))

    _condition(z_of, slabs[0] if summed else x)
    shifted = {_pick(case, ["x", "x2", "y"])} if not case.align[0] else set()

    def launch():
        d, d2 = p.dev(dev), p2.dev(dev)
        xin = _nan(shape, dev, "x" in shifted) if summed else _put(x, dev, "x" in shifted)
        x2in = _nan(shape, dev, "x2" in shifted) if summed2 else _put(x2, dev, "x2" in shifted)
        y = _nan(shape, dev, "y" in shifted)
        xpart = _put(slabs, dev, not case.align[2]) if slabs is not None else None
        x2part = _put(slabs2, dev, not case.align[3]) if slabs2 is not None else None
        al = (_a16(xin, x2in, y), True, _a16(xpart if summed else None), _a16(x2part if summed2 else None))
        _premise(X, case, al)
        _pair_fwd_call(X, d, d2, xin, x2in, y, xpart, ns, x2part, ns2)
        return _cpu(y=y, x=xin, x2=x2in, save_mean=d["sm"], save_invstd=d["si"], running_mean=d["rmean"],
                    running_var=d["rvar"], num_batches_tracked=d["nbt"], save_mean2=d2["sm"], save_invstd2=d2["si"],
                    running_mean2=d2["rmean"], running_var2=d2["rvar"], num_batches_tracked2=d2["nbt"])

    o = _twice(launch)
    if summed:
        _check_sum(o["x"], slabs, None, "summed x")
    if summed2:
        _check_sum(o["x2"], slabs2, None, "summed x2")
    z = z_of(o["x"], o["x2"])
    assert torch.equal(o["y"] > 0, z > 0), "the device ReLU mask differs from the fp64 mask"
    _near(o["y"], torch.relu(z), "y", 1e-5, 2e-5)
    _check_fwd_stats(o, p, *_batch_stats(o["x"].double()), N * HW)
    _check_fwd_stats(o, p2, *_batch_stats(o["x2"].double()), N * HW, "2")


def _check_pair_bwd(X, dev, case):
    C, ns, addend = case.C, case.nslab, bool(case.addend)
    shape, p, p2, x, x2 = _pair_inputs(case, _Rng(case.id))
    x2d = x2.double()

    def z_of():
        xd = x.double()
        return _bn(xd, p, *_batch_stats(xd)) + _bn(x2d, p2, *_batch_stats(x2d))

    _condition(z_of, x)
    xd = x.double()
    mask = z_of() > 0
    rng = _Rng(case.id + "/dy")
    dy = rng(*shape)
    slabs = _slabs(rng, dy, ns)
    summed = ns >= 2
    dyadd = rng(*shape) if addend else None
    shifted = {_pick(case, ["x", "dy", "y", "dx", "x2", "dx2"])} if not case.align[0] else set()
    if not case.align[2]:
        shifted.add(_pick(case, ["slabs"] + (["dyadd"] if addend else [])))

    def launch():
        d, d2 = p.dev(dev), p2.dev(dev)
        y = _nan(shape, dev)
        _pair_fwd_call(X, d, d2, _put(x, dev), _put(x2, dev), y)  # the forward that the backward follows
        assert torch.equal(y.cpu() > 0, mask), "the device ReLU mask differs from the fp64 mask"
        xin, x2in = _put(x, dev, "x" in shifted), _put(x2, dev, "x2" in shifted)
        yin = _put(y.cpu(), dev, "y" in shifted)
        dyin = _nan(shape, dev, "dy" in shifted) if summed else _put(dy, dev, "dy" in shifted)
        dypart = _put(slabs, dev, "slabs" in shifted) if slabs is not None else None
        add = _put(dyadd, dev, "dyadd" in shifted) if addend else None
        dx, dx2 = _nan(shape, dev, "dx" in shifted), _nan(shape, dev, "dx2" in shifted)
        g = [_nan((C,), dev) for _ in range(4)]
        al = (_a16(xin, dyin, yin, dx, x2in, dx2), True, _a16(dypart if summed else None, add), True)
        _premise(X, case, al)
        X.bn_pair_bwd(dyin, yin, xin, x2in, d["gamma"], d["sm"], d["si"], d2["gamma"], d2["sm"], d2["si"], dx, dx2,
                      g[0], g[1], g[2], g[3], dypart, ns, add)
        return _cpu(dx=dx, dx2=dx2, dgamma=g[0], dbeta=g[1], dgamma2=g[2], dbeta2=g[3], dy=dyin, y=y)

    o = _twice(launch)
    dz = _summed_dy(case, o["dy"], slabs, dyadd) * mask
    for sfx, pp, xx in (("", p, xd), ("2", p2, x2d)):
        dx, dgamma, dbeta = _bn_bwd(dz, xx, pp, *_batch_stats(xx))
        _near(o["dx" + sfx], dx, "dx" + sfx, 1e-4, 5e-5)
        _near(o["dgamma" + sfx], dgamma, "dgamma" + sfx, 1e-5, 1e-4)
        _near(o["dbeta" + sfx], dbeta, "dbeta" + sfx, 1e-5, 1e-4)


# ----------------------------------------- the stem tail -------------------------------------
def _windows(a):
    """[N, C, 9, OH * OW]: the taps of every 3x3 / stride 2 / pad 1 window, -inf outside the map"""
    N, C = a.shape[:2]
    return F.unfold(F.pad(a, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).view(N, C, 9, -1)


def _check_stem(X, dev, case):
    N, C, W = case.N, case.C, case.pool_w
    shape, OW = (N, C, W, W), (W - 1) // 2 + 1
    rng = _Rng(case.id)
    p = _Params(rng, C)
    x = rng(*shape, scale=1.7, bias=0.4)

    def z_of():
        xd = x.double()
        return _bn(xd, p, *_batch_stats(xd))

    def ties(z):
        """the elements that are a window's positive maximum with a second tap within MARGIN of it"""
        a = torch.relu(z)
        top = _windows(a).topk(2, dim=2).values
        tie = ((top[:, :, 0] > 0) & (top[:, :, 0] - top[:, :, 1] < MARGIN)).to(torch.int8)
        where = F.max_pool2d(a, 3, 2, 1, return_indices=True)[1].flatten(2)
        return torch.zeros(N, C, W * W, dtype=torch.int8).scatter_reduce_(2, where, tie, "amax").view(shape).bool()

    # every window's maximum is unique or zero: the winning tap is raised (z moves with sign(gamma))
    _condition(z_of, x, sign=torch.sign(p.gamma).view(1, C, 1, 1), extra=ties)
    xst = _ext_stats(x.double(), x.double(), case.ext_slices) if case.ext_slices else None
    shift = _misaligned(case)

    def launch():
        d = p.dev(dev)
        xin = _put(x, dev, shift)
        y = _nan((N, C, OW, OW), dev)
        idx = torch.full((N, C, OW, OW), 255, dtype=torch.uint8, device=dev)
        st = _put(xst, dev) if xst is not None else None
        route = _premise(X, case, (True, _a16(xin), True, True))
        X.bn_relu_maxpool(xin, y, idx, d["gamma"], d["beta"], d["rmean"], d["rvar"], d["nbt"], d["sm"], d["si"],
                          _part(route, dev), EPS, MOM, st, case.ext_slices if st is not None else 0)
        return _cpu(y=y, idx=idx, save_mean=d["sm"], save_invstd=d["si"], running_mean=d["rmean"],
                    running_var=d["rvar"], num_batches_tracked=d["nbt"])

    o = _twice(launch)
    xd = x.double()
    a = torch.relu(z_of())
    want, where = F.max_pool2d(a, 3, 2, 1, return_indices=True)
    err = (o["y"].double() - want).abs().max().item()
    print(f"pooled y: max abs err {err:.3e}")
    assert err <= 1e-4 * (want.abs().max().item() + 1e-12), ("pooled y", err)  # (nan fails)
    oh = torch.arange(OW).view(1, 1, OW, 1)
    ow = torch.arange(OW).view(1, 1, 1, OW)
    tap = (torch.div(where, W, rounding_mode="floor") - (2 * oh - 1)) * 3 + (where % W - (2 * ow - 1))
    live = want > 0
    assert torch.equal(o["idx"].long()[live], tap[live]), "the winning tap differs where the pooled value is positive"
    _check_fwd_stats(o, p, *_batch_stats(xd), N * W * W)


# -------------------------------------------- tests ------------------------------------------
def _ext():
    from network_distributed_pytorch_amd.ops import ext, native_available

    assert native_available(), "native extension missing"
    return ext()


def _run(X, dev, case):
    if case.kind in ("bn_fwd", "bn_bwd"):
        check = _check_bn_fwd if case.kind == "bn_fwd" else _check_bn_bwd
        for res, relu in ARMS:
            if case.mbeta and (res or not relu):
                continue  # the mask recomputed from x: relu, and no residual behind the mask
            check(X, dev, case, res, relu)
    else:
        {"pair_fwd": _check_pair_fwd, "pair_bwd": _check_pair_bwd, "stem_fwd": _check_stem}[case.kind](X, dev, case)


@pytest.mark.parametrize("case", R.cases(), ids=lambda c: c.id)
def test_bn_route_vs_fp64(device, case):
    _run(_ext(), device, case)


@pytest.mark.parametrize("HW", R.SWITCH_OFF_HWS)
def test_bn_float4_switch_off_vs_fp64(device, HW):
    """bn_set_vec4(False), a shipped knob: one forward and one backward per map size, the premise
    taken from the table's float4-off rows"""
    X = _ext()
    X.bn_set_vec4(False)
    try:
        for case in R.switch_off_cases(HW):
            _run(X, device, case)
    finally:
        X.bn_set_vec4(True)
