"""Grad-W operand pipelining (fusion ``wgrad_pipe``): the layer1 Winograd grad-W's LDS prefetch of
the next image (csrc/winograd.hip) and the 4-image stages of the layer2 3x3 class's direct grad-W
(csrc/conv.hip; the 3x3/2 and 1x1/2 classes keep the one-image loop and are here to show that).
Both keep every accumulator's MFMA order, so grad-W is bitwise what the one-image loops give; it
is also held against an fp64 CPU oracle with the bounds of tests/test_conv_direct.py.  The batches
are the smallest that reach each slice / stage shape through conv_wgrad_imgs."""
import pytest
import torch
import torch.nn.functional as F

# (cin, cout, k, stride, pad, hw, batch)
WINO = [(cin, 64, 3, 1, 1, 8, B) for cin in (64, 128) for B in (8, 64, 128, 264, 512, 520)]
CLS1 = [(128, 128, 3, 1, 1, 4, B) for B in (16, 32, 64, 128, 256, 512)]
CLS2 = [(64, 128, 3, 2, 1, 8, B) for B in (64, 256, 512)]
CLS45 = [(64, 128, 1, 2, 0, 8, B) for B in (64, 512)] + [(128, 256, 1, 2, 0, 4, B) for B in (64, 512)]
CASES = WINO + CLS1 + CLS2 + CLS45

_DATA: dict = {}


def _case(case, device):
    """x, dy on the device and the fp64 grad-W of the case, computed once and never modified."""
    if case not in _DATA:
        cin, cout, k, s, p, hw, B = case
        g = torch.Generator().manual_seed(11)
        x = torch.randn(B, cin, hw, hw, generator=g)
        oh = (hw + 2 * p - k) // s + 1
        dy = torch.randn(B, cout, oh, oh, generator=g)
        w = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
        F.conv2d(x.double(), w, stride=s, padding=p).backward(dy.double())
        _DATA[case] = (x.to(device), dy.to(device), w.grad.detach())
    return _DATA[case]


def _pipe(on):
    """Both halves of the switch: True = pipelined where the slice allows, False = the one-image loops."""
    from network_distributed_pytorch_amd.ops._ext import ext

    ext().conv_set_wgrad_stage(0 if on else 1)
    ext().wino_set_wgrad_prefetch(bool(on))


def _restore():
    from network_distributed_pytorch_amd.knobs import fusion_on
    from network_distributed_pytorch_amd.ops._ext import ext

    ext().conv_set_wgrad_stage(0)
    ext().wino_set_wgrad_prefetch(fusion_on("wgrad_pipe"))


def _dw(case, x, dy):
    from network_distributed_pytorch_amd.ops._ext import ext
    from network_distributed_pytorch_amd.ops.conv import direct_plan

    cin, cout, k, s, p, hw, B = case
    w = torch.empty(cout, cin, k, k, device=x.device)
    plan = direct_plan(x, w, s, p)
    assert plan is not None
    part = torch.empty((B // plan[2]) * w.numel(), device=x.device)
    dw = torch.empty_like(w)
    ext().conv_wgrad(x, dy, part, dw, list(plan[0]))
    return dw


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_wgrad_pipe_is_bitwise(device, case):
    """dw with the pipelined feeding == dw with the one-image loops, and run to run."""
    x, dy, _ = _case(case, device)
    try:
        _pipe(True)
        on = _dw(case, x, dy)
        _pipe(False)
        off = _dw(case, x, dy)
        _pipe(True)
        again = _dw(case, x, dy)
    finally:
        _restore()
    assert torch.equal(on, off)
    assert torch.equal(on, again)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_wgrad_pipe_vs_fp64(device, case):
    cin, cout, k, s, p, hw, B = case
    x, dy, ref = _case(case, device)
    try:
        _pipe(True)
        dw = _dw(case, x, dy).double().cpu()
    finally:
        _restore()
    err = (dw - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"{case}: err {err:.3e} scale {scale:.3e} rel {err / scale:.3e}")
    if k == 3 and s == 1 and hw == 8:  # the Winograd grad-W (tests/test_conv_direct.py:179)
        assert err / scale <= 4e-6 * (cin * 9) ** 0.5, (err, scale)
    else:  # the direct classes (tests/test_conv_direct.py:40)
        assert err <= 2e-6 * scale * (cin * k * k) ** 0.5 + 1e-6, (err, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout,hw,B", [(64, 64, 8, 64), (64, 64, 8, 512), (128, 128, 4, 64), (128, 128, 4, 512)])
def test_wgrad_pipe_through_the_pairs(device, cin, cout, hw, B):
    """One 3x3 conv's backward with pairing on (grad-W held back, launched with its grad-x:
    wino_bwd_pair_kernel for layer1, wino_direct_pair_kernel for layer2): dx, the grad-W slabs and
    dw are bitwise the same with ``wgrad_pipe`` on and off, and each backward makes exactly one
    pair launch.  At B = 64 the slices are too short to pipeline (one image per wave, 4-image
    slices), so both arms run the one-image loops there; B = 512 runs the new feeding in the pairs."""
    from network_distributed_pytorch_amd.ops._ext import ext
    from network_distributed_pytorch_amd.ops.conv import direct_plan

    g = torch.Generator().manual_seed(12)
    x = torch.randn(B, cin, hw, hw, generator=g).to(device)
    dy = torch.randn(B, cout, hw, hw, generator=g).to(device)
    w = (torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5).to(device)
    plan = direct_plan(x, w, 1, 1)
    assert plan is not None
    geom, slices, ksd = list(plan[0]), B // plan[2], plan[5]
    assert bool(ext().conv_wino(geom, B, True)), "grad-x should take the Winograd kernel (the pair needs it)"
    wu = torch.empty(32 * w.numel() // 9, device=device)
    ext().wino_weights(w, wu)

    def backward():
        part_w = torch.zeros(slices * w.numel(), device=device)
        pairs = ext().conv_pair_launches()
        ext().conv_wgrad(x, dy, part_w, None, geom, True)  # held back for the grad-x below
        dx = torch.empty_like(x)
        part_x = torch.empty(ksd * x.numel(), device=device) if ksd > 1 else None
        assert ext().conv_dgrad(dy, w, dx, geom, part_x, None, False, wino_u=wu) == 1
        assert ext().conv_pair_launches() == pairs + 1, "the grad-W should have run in the grad-x launch"
        ext().conv_flush_pending()
        dw = torch.empty_like(w)
        ext().slab_sum(part_w, dw, slices)
        return dx, part_w, dw

    try:
        _pipe(True)
        on = backward()
        _pipe(False)
        off = backward()
    finally:
        _restore()
    for a, b, name in zip(on, off, ("dx", "slabs", "dw")):
        assert torch.equal(a, b), name


@pytest.mark.gpu
def test_wgrad_stage_rejects_unbuilt_values(device):
    """Only 0 (auto), 1 and 4 images per stage exist; anything else must not pass for one of them."""
    from network_distributed_pytorch_amd.ops._ext import ext

    try:
        for n in (2, 3, 8, -1):
            with pytest.raises(RuntimeError):
                ext().conv_set_wgrad_stage(n)
        for n in (1, 4, 0):
            ext().conv_set_wgrad_stage(n)
    finally:
        _restore()
