"""csrc/loss.hip: ce_soft_fwd_kernel (label smoothing, two weighted targets per row) against the fp64
formula of tests/soft_loss_rule.py, with the tolerances of tests/test_loss_gpu.py; the default call
stays bitwise the plain kernel; run-to-run and hipGraph-replay determinism; the running sum."""
import pytest
import torch

from network_distributed_pytorch_amd import ops
from network_distributed_pytorch_amd.ops.loss import CrossEntropyLoss, cross_entropy

from .soft_loss_rule import soft_case, soft_ce_fp64

pytestmark = pytest.mark.gpu

# K = 1100 takes the looping path, B = 333 leaves a partial last workgroup
SHAPES = [(1, 7), (16, 2), (333, 10), (64, 1000), (9, 1100)]


@pytest.mark.parametrize("B,K", SHAPES)
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("with_b", [False, True])
def test_soft_cross_entropy_matches_fp64(device, B, K, eps, with_b):
    assert ops.native_available()
    x, ta, tb, lam = soft_case(B, K, device, with_b)
    x = x.requires_grad_(True)
    x64 = x.detach().double().requires_grad_(True)
    ref = soft_ce_fp64(x64, ta, eps, tb, lam)
    if eps == 0.0 and not with_b:  # the call the front-end keeps on ce_fwd_kernel: ask the binding directly
        loss = _native_soft(x, ta, eps, None, None)
    else:
        loss = cross_entropy(x, ta, label_smoothing=eps, target_b=tb, lam=lam)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    print(f"B={B} K={K} eps={eps} b={with_b}: loss err {abs(float(loss.detach()) - float(ref.detach())):.3e}")
    torch.testing.assert_close(loss.double(), ref, rtol=2e-6, atol=2e-6)
    g = torch.tensor(1.7, device=device)
    (loss * g).backward()
    (ref * g.double()).backward()
    print(f"  grad err {float((x.grad.double() - x64.grad).abs().max()):.3e}")
    torch.testing.assert_close(x.grad.double(), x64.grad, rtol=1e-5, atol=1e-7)
    if B > 8:
        assert float(x.grad[ta == -100].abs().max()) == 0  # ignored rows: zero gradient


def _native_soft(x, ta, eps, tb, lam):
    from network_distributed_pytorch_amd.ops.loss import _SoftCrossEntropyFn

    return _SoftCrossEntropyFn.apply(x, ta, -100, None, eps, tb, lam)


@pytest.mark.parametrize("B,K", [(333, 10), (9, 1100)])
def test_default_call_is_bitwise_the_plain_kernel(device, B, K):
    x, ta, _, _ = soft_case(B, K, device, False)
    xa = x.clone().requires_grad_(True)
    xb = x.clone().requires_grad_(True)
    a = cross_entropy(xa, ta)
    b = cross_entropy(xb, ta, label_smoothing=0.0, target_b=None, lam=None)
    assert torch.equal(a, b)
    (a * 1.7).backward()
    (b * 1.7).backward()
    assert torch.equal(xa.grad, xb.grad)
    # the soft kernel at eps = 0 with one target computes the same loss (to rounding: another kernel)
    torch.testing.assert_close(_native_soft(x, ta, 0.0, None, None), a, rtol=2e-6, atol=2e-6)
    crit = CrossEntropyLoss()
    assert torch.equal(crit(x, ta), a)


def test_out_of_range_target_gives_nan_and_ignored_rows_nothing(device):
    x, ta, tb, lam = soft_case(16, 5, device, True)
    bad_b = tb.clone()
    bad_b[1] = 5
    assert torch.isnan(cross_entropy(x, ta, label_smoothing=0.1, target_b=bad_b, lam=lam))
    bad_a = ta.clone()
    bad_a[1] = -3
    assert torch.isnan(cross_entropy(x, bad_a, label_smoothing=0.1))
    assert torch.isfinite(cross_entropy(x, ta, label_smoothing=0.1, target_b=tb, lam=lam))
    with pytest.raises(RuntimeError, match="label_smoothing"):
        ops.ext().ce_soft_fwd(x, ta, torch.empty_like(x), torch.empty(17, device=device),
                              torch.empty((), device=device), torch.zeros(1, dtype=torch.int32, device=device),
                              -100, 1.0)
    with pytest.raises(RuntimeError, match="together"):
        ops.ext().ce_soft_fwd(x, ta, torch.empty_like(x), torch.empty(17, device=device),
                              torch.empty((), device=device), torch.zeros(1, dtype=torch.int32, device=device),
                              -100, 0.1, tb)


def test_soft_cross_entropy_deterministic_and_graph_safe(device):
    x, ta, tb, lam = soft_case(256, 1000, device, True)
    crit = CrossEntropyLoss(label_smoothing=0.1)
    a = [crit(x, ta, tb, lam) for _ in range(3)]
    assert all(torch.equal(a[0], v) for v in a)
    xe = x.clone().requires_grad_(True)
    crit(xe, ta, tb, lam).backward()
    xs = x.clone().requires_grad_(True)
    out = torch.zeros((), device=device)
    crit(xs, ta, tb, lam).backward()  # warm-up (eager) allocates the counter
    xs.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss = crit(xs, ta, tb, lam)
        loss.backward()
        out.copy_(loss)
    for _ in range(3):
        xs.grad.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, a[0])
        assert torch.equal(xs.grad, xe.grad)
    # the plain kernel shares the counter: it still runs after the soft one, bitwise itself
    plain = [cross_entropy(x, ta) for _ in range(2)]
    assert torch.equal(plain[0], plain[1]) and torch.isfinite(plain[0])


def test_soft_cross_entropy_accumulates_running_sum(device):
    acc = torch.zeros((), device=device)
    crit = CrossEntropyLoss(label_smoothing=0.1)
    crit.accumulate = acc
    ref = torch.zeros((), device=device)
    for i in range(3):
        x, ta, tb, lam = soft_case(64, 1000, device, True, seed=i)
        x = x.requires_grad_(True)
        loss = crit(x, ta, tb, lam)
        plain = cross_entropy(x.detach(), ta, label_smoothing=0.1, target_b=tb, lam=lam)
        assert torch.equal(loss.detach(), plain)
        ref += plain
        loss.backward()
        assert torch.isfinite(x.grad).all()
    torch.cuda.synchronize()
    assert torch.equal(acc, ref)
