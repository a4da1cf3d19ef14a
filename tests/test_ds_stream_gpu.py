"""The streamed 1x1 stride-2 downsample bodies (fusion ``ds_stream``, csrc/ds_stream.h): forward,
grad-x and grad-W of the kConv1x1S2Map8 / kConv1x1S2Map4 classes as GEMMs fed from registers.  The
bodies keep the summation order of conv_fwd_body and conv_wgrad_body (the same MFMA steps on every
accumulator, in the same order), so every result — outputs, split-K slabs, grad-W slabs — is
bitwise the old bodies' (``test_ds_stream_is_bitwise_the_old_bodies``).  Each direction is also held
against an fp64 oracle with the bound "twice the old body's own error on the same inputs", and the
structure the consumers rely on is checked bitwise: odd pixels of the grad-x, the split-K slabs,
the pair launches against the bodies alone, and run-to-run repeatability.  (The 8x8 forward runs
conv_fwd_body in both arms.)

Measured maximum absolute errors against fp64 (old body / streamed body) are printed by
``test_ds_stream_vs_fp64`` and recorded in profiles/r11/README.md."""
import pytest
import torch
import torch.nn.functional as F

# (cin, cout, hw, batch): the layer2 / layer3 downsamples at the batches where the plan changes
# (N = 64: split-K 4 in both directions), and the wide geometries of the classes once each
DS2 = [(64, 128, 8, N) for N in (4, 8, 64)]
DS3 = [(128, 256, 4, N) for N in (16, 32, 64)]
WIDE = [(256, 512, 8, 4), (512, 1024, 4, 16)]
CASES = DS2 + DS3 + WIDE
_ID = lambda c: "x".join(map(str, c))  # noqa: E731

_DATA: dict = {}


def _case(case, device):
    """Seeded x, w, dy, addend on the device and the fp64 y, dx, dw: computed once, never modified."""
    if case not in _DATA:
        cin, cout, hw, B = case
        g = torch.Generator().manual_seed(23)
        x = torch.randn(B, cin, hw, hw, generator=g)
        w = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
        dy = torch.randn(B, cout, hw // 2, hw // 2, generator=g)
        add = torch.randn(B, cin, hw, hw, generator=g)
        xd = x.double().requires_grad_(True)
        wd = w.double().requires_grad_(True)
        y = F.conv2d(xd, wd, stride=2)
        y.backward(dy.double())
        _DATA[case] = dict(x=x.to(device), w=w.to(device), dy=dy.to(device), add=add.to(device),
                           y=y.detach(), dx=xd.grad.detach(), dw=wd.grad.detach())
    return _DATA[case]


def _stream(on):
    from network_distributed_pytorch_amd.ops._ext import ext

    ext().conv_set_ds_stream(1 if on else 0)


def _restore():
    from network_distributed_pytorch_amd.ops._ext import ext

    ext().conv_set_ds_stream(-1)  # by NDP_FUSION_OFF again


def _plan(d):
    from network_distributed_pytorch_amd.ops.conv import direct_plan

    plan = direct_plan(d["x"], d["w"], 2, 0)
    assert plan is not None
    return plan


def _fwd(d, defer=False):
    """y (unwritten when the slabs are left), the split-K scratch and the slabs left in it"""
    from network_distributed_pytorch_amd.ops._ext import ext

    plan = _plan(d)
    y = torch.full_like(d["dy"], float("nan"))
    part = torch.empty(plan[4] * y.numel(), device=y.device) if plan[4] > 1 else None
    left = ext().conv_fwd(d["x"], d["w"], y, list(plan[0]), part, defer)
    return y, part, left


def _dgrad(d, addend=None):
    """dx and the split-K scratch (compact slabs, summed by the launcher: the class cannot defer)"""
    from network_distributed_pytorch_amd.ops._ext import ext

    plan = _plan(d)
    dx = torch.full_like(d["x"], float("nan"))
    cin, cout = d["x"].shape[1], d["dy"].shape[1]
    part = torch.empty(plan[5] * (d["dy"].numel() // cout) * cin, device=dx.device) if plan[5] > 1 else None
    assert ext().conv_dgrad(d["dy"], d["w"], dx, list(plan[0]), part, addend, False) == 1
    return dx, part


def _wgrad(d):
    from network_distributed_pytorch_amd.ops._ext import ext

    plan = _plan(d)
    B = d["x"].shape[0]
    part = torch.empty((B // plan[2]) * d["w"].numel(), device=d["x"].device)
    dw = torch.empty_like(d["w"])
    ext().conv_wgrad(d["x"], d["dy"], part, dw, list(plan[0]))
    return dw


def _three(d):
    return {"y": _fwd(d)[0], "dx": _dgrad(d)[0], "dw": _wgrad(d)}


def _err(got, ref):
    return (got.double().cpu() - ref).abs().max().item()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_ID)
def test_ds_stream_vs_fp64(device, case):
    """Forward, grad-x and grad-W against float64 conv2d and its autograd: the streamed bodies' maximum
    absolute error stays within twice the old bodies' on the same inputs."""
    d = _case(case, device)
    try:
        _stream(False)
        old = _three(d)
        _stream(True)
        new = _three(d)
    finally:
        _restore()
    for k in ("y", "dx", "dw"):
        e_old, e_new = _err(old[k], d[k]), _err(new[k], d[k])
        print(f"{_ID(case)} {k}: old {e_old:.3e} new {e_new:.3e} scale {d[k].abs().max().item():.3e}")
    for k in ("y", "dx", "dw"):
        e_old, e_new = _err(old[k], d[k]), _err(new[k], d[k])
        assert e_new <= 2 * e_old, (k, e_new, e_old)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES + [(64, 128, 8, 512), (128, 256, 4, 512)], ids=_ID)
def test_ds_stream_is_bitwise_the_old_bodies(device, case):
    """y, dx (with and without addend), dw and the split-K scratch of both directions: streamed ==
    conv_fwd_body / conv_wgrad_body, bit for bit."""
    d = _case(case, device)

    def run():
        y, ypart, _ = _fwd(d, defer=True)
        dx, dpart = _dgrad(d)
        out = {"y": _fwd(d)[0], "dx": dx, "dxa": _dgrad(d, d["add"])[0], "dw": _wgrad(d)}
        if ypart is not None:
            out["ypart"] = ypart
        if dpart is not None:
            out["dpart"] = dpart
        return out

    try:
        _stream(False)
        old = run()
        _stream(True)
        new = run()
    finally:
        _restore()
    assert old.keys() == new.keys()
    for k in old:
        assert torch.equal(old[k], new[k]), k


@pytest.mark.gpu
def test_ds_stream_ragged_batch(device):
    """N = 20 on the 4x4 class: no tile of the plan divides it, so it runs zero-padded to 32 images
    (ops/conv.py direct_plan_padded) on the same kernels; all three directions against fp64 within
    twice the old bodies' error."""
    from network_distributed_pytorch_amd.ops.conv import DirectConvFn, direct_plan, direct_plan_padded

    cin, cout, hw, B = 128, 256, 4, 20
    g = torch.Generator().manual_seed(29)
    x = torch.randn(B, cin, hw, hw, generator=g)
    w = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    dy = torch.randn(B, cout, hw // 2, hw // 2, generator=g)
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    ref_y = F.conv2d(xd, wd, stride=2)
    ref_y.backward(dy.double())
    ref = {"y": ref_y.detach(), "dx": xd.grad, "dw": wd.grad}

    def run():
        xg, wg = x.to(device).requires_grad_(True), w.to(device).requires_grad_(True)
        assert direct_plan(xg, wg, 2, 0) is None
        plan, Bp = direct_plan_padded(xg, wg, 2, 0)
        xp = torch.cat([xg, xg.new_zeros((Bp - B,) + tuple(xg.shape[1:]))])
        y = DirectConvFn.apply(xp, wg, plan, None, None, None)[:B]
        y.backward(dy.to(device))
        return {"y": y.detach(), "dx": xg.grad, "dw": wg.grad}

    try:
        _stream(False)
        old = run()
        _stream(True)
        new = run()
    finally:
        _restore()
    for k in ("y", "dx", "dw"):
        e_old, e_new = _err(old[k], ref[k]), _err(new[k], ref[k])
        print(f"128x256x4x20 {k}: old {e_old:.3e} new {e_new:.3e}")
        assert e_new <= 2 * e_old, (k, e_new, e_old)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [DS2[0], DS2[2], DS3[0], DS3[2], WIDE[0]], ids=_ID)
def test_ds_stream_dgrad_odd_pixels(device, case):
    """Without an addend every odd pixel of dx is exactly 0; with one it is bitwise the addend's
    value, and the even pixels are the addend plus the product (one rounding)."""
    d = _case(case, device)
    try:
        _stream(True)
        plain = _dgrad(d)[0]
        added = _dgrad(d, d["add"])[0]
    finally:
        _restore()
    odd = torch.ones_like(plain, dtype=torch.bool)
    odd[:, :, ::2, ::2] = False
    assert torch.count_nonzero(plain[odd]).item() == 0
    assert torch.equal(added[odd], d["add"][odd])
    assert torch.equal(added[:, :, ::2, ::2], plain[:, :, ::2, ::2] + d["add"][:, :, ::2, ::2])


@pytest.mark.gpu
@pytest.mark.parametrize("case", [DS2[2], DS3[2]], ids=_ID)
def test_ds_stream_split_k_slabs(device, case):
    """N = 64 (split-K 4 in both directions): the forward slabs left to the consumer (defer) and the
    compact grad-x slabs, added in z order, are bitwise the result the launcher's own sum gives."""
    d = _case(case, device)
    plan = _plan(d)
    assert plan[4] == 4 and plan[5] == 4
    try:
        _stream(True)
        y, _, left = _fwd(d)
        assert left == 1
        _, part, left = _fwd(d, defer=True)
        assert left == 4
        dx, dpart = _dgrad(d)
    finally:
        _restore()
    s = part.view(4, *y.shape)
    assert torch.equal(((s[0] + s[1]) + s[2]) + s[3], y)
    B, cin, hw, _ = d["x"].shape
    s = dpart.view(4, B, cin, hw // 2, hw // 2)
    assert torch.equal(((s[0] + s[1]) + s[2]) + s[3], dx[:, :, ::2, ::2])


@pytest.mark.gpu
@pytest.mark.parametrize("case", [DS2[1], DS2[2], (64, 128, 8, 512), DS3[2], (128, 256, 4, 512)], ids=_ID)
def test_ds_stream_bwd_pair_is_bitwise(device, case):
    """The grad-x in one launch with the held-back grad-W (direct_pair_kernel) == the two bodies
    launched alone, with and without an addend; exactly one pair launch."""
    from network_distributed_pytorch_amd.ops._ext import ext

    d = _case(case, device)
    plan = _plan(d)
    geom, slices = list(plan[0]), d["x"].shape[0] // plan[2]
    cin, cout = d["x"].shape[1], d["dy"].shape[1]

    def pair(addend):
        part_w = torch.zeros(slices * d["w"].numel(), device=device)
        n = ext().conv_pair_launches()
        ext().conv_wgrad(d["x"], d["dy"], part_w, None, geom, True)  # held back for the grad-x below
        dx = torch.full_like(d["x"], float("nan"))
        part_x = torch.empty(plan[5] * (d["dy"].numel() // cout) * cin, device=device) if plan[5] > 1 else None
        assert ext().conv_dgrad(d["dy"], d["w"], dx, geom, part_x, addend, False) == 1
        assert ext().conv_pair_launches() == n + 1, "the grad-W should have run in the grad-x launch"
        ext().conv_flush_pending()
        dw = torch.empty_like(d["w"])
        ext().slab_sum(part_w, dw, slices)
        return dx, dw

    try:
        _stream(True)
        for addend in (None, d["add"]):
            dx, dw = pair(addend)
            assert torch.equal(dx, _dgrad(d, addend)[0])
            assert torch.equal(dw, _wgrad(d))
    finally:
        _restore()


@pytest.mark.gpu
@pytest.mark.parametrize("B", [8, 64, 512])
def test_ds_stream_fwd_pair_is_bitwise(device, B):
    """The downsample forward held back and launched with the block's 3x3 stride-2 conv1
    (ds_fwd_pair_kernel) == both convs launched alone."""
    from network_distributed_pytorch_amd.ops._ext import ext
    from network_distributed_pytorch_amd.ops.conv import direct_plan

    g = torch.Generator().manual_seed(31)
    x = torch.randn(B, 64, 8, 8, generator=g).to(device)
    w1 = (torch.randn(128, 64, 3, 3, generator=g) / 24).to(device)
    wd = (torch.randn(128, 64, 1, 1, generator=g) / 8).to(device)
    p1, pd = direct_plan(x, w1, 2, 1), direct_plan(x, wd, 2, 0)

    def run(pair):
        out = []
        for w, plan, hold in ((wd, pd, pair), (w1, p1, False)):  # the downsample first: it is the one held
            y = torch.full((B, 128, 4, 4), float("nan"), device=device)
            part = torch.empty(plan[4] * y.numel(), device=device) if plan[4] > 1 else None
            assert ext().conv_fwd(x, w, y, list(plan[0]), part, False, None, None, hold) == 1
            out.append((y, part))
        ext().conv_flush_pending_fwd()
        return [y for y, _ in out]

    try:
        _stream(True)
        yd, y1 = run(True)
        ad, a1 = run(False)
    finally:
        _restore()
    assert torch.equal(yd, ad) and torch.equal(y1, a1)
    assert not torch.isnan(yd).any() and not torch.isnan(y1).any()


@pytest.mark.gpu
@pytest.mark.parametrize("case", [DS2[2], DS3[2], WIDE[1]], ids=_ID)
def test_ds_stream_repeatable(device, case):
    """Two runs on the same inputs: bitwise equal in all three directions."""
    d = _case(case, device)
    try:
        _stream(True)
        a, b = _three(d), _three(d)
    finally:
        _restore()
    for k in ("y", "dx", "dw"):
        assert torch.equal(a[k], b[k]), k


def test_ds_stream_knob_is_listed():
    from network_distributed_pytorch_amd.knobs import FUSIONS, fusion_on

    assert "ds_stream" in FUSIONS and isinstance(fusion_on("ds_stream"), bool)
