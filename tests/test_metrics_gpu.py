"""Fused classification metrics (csrc/loss.hip cls_metrics_kernel) against a CPU reference of
the stated rule: counts exact, loss sum within the loss test's per-row tolerance, summed."""
import pytest
import torch

from network_distributed_pytorch_amd import ops
from network_distributed_pytorch_amd.ops.metrics import classification_metrics

from .metric_rule import loss_sum_fp64, rule_counts

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2), (5, 7), (64, 10), (67, 1000), (16, 1024), (16, 1025), (1029, 129)]


def _targets(B, K, device):
    t = torch.randint(0, K, (B,), device=device)
    if B > 8:
        t[::7] = -100  # ignored rows
    return t


def _check(x, t, k):
    pred = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    state = classification_metrics(x, t, k=k, pred=pred).cpu()
    n, c1, ck = rule_counts(x, t, k)
    print(f"shape={tuple(x.shape)} k={k} state={state.tolist()} rule=({n}, {c1}, {ck})")
    assert state.dtype == torch.float64
    assert state[1:].tolist() == [float(n), float(c1), float(ck)]
    return state, pred.cpu(), n


@pytest.mark.parametrize("B,K", SHAPES)
def test_metrics_match_rule(device, B, K):
    assert ops.native_available()
    torch.manual_seed(B * 7 + K)
    x = torch.randn(B, K, device=device) * 3
    t = _targets(B, K, device)
    # lift the target's logit by a random amount, so that ranks 0, 1..4 and beyond all occur
    rows = torch.arange(B, device=device)
    x[rows, t.clamp(min=0)] += torch.rand(B, device=device) * 9
    for k in ([1, 5] if K >= 5 else [1, K]):
        state, pred, n = _check(x, t, k)
        ref = loss_sum_fp64(x, t)
        assert abs(float(state[0]) - ref) <= 2e-6 * abs(ref) + 2e-6 * n, (float(state[0]), ref)
        want = torch.where(t.cpu() != -100, x.cpu().argmax(dim=1), torch.full_like(t.cpu(), -100))
        assert torch.equal(pred, want)


@pytest.mark.parametrize("B,K", [(64, 10), (16, 1500)])
def test_metrics_ties_are_deterministic(device, B, K):
    torch.manual_seed(B + K)
    x = torch.randint(-2, 3, (B, K), device=device).float()
    t = _targets(B, K, device)
    # targets near the row's start that hold the maximum: their rank is the number of EARLIER
    # equal entries, so top-1 / top-5 hinge on the tie rule
    early = torch.arange(0, B, 3, device=device)
    t[early] = torch.randint(0, 12 if K > 12 else K, (early.numel(),), device=device)
    x[early, t[early]] = 2.0
    for k in (1, 5):
        state, pred, n = _check(x, t, k)
        ref = loss_sum_fp64(x, t)
        assert abs(float(state[0]) - ref) <= 2e-6 * abs(ref) + 2e-6 * n
        want = torch.where(t.cpu() != -100, x.cpu().argmax(dim=1), torch.full_like(t.cpu(), -100))
        assert torch.equal(pred, want)


@pytest.mark.parametrize("K", [10, 1500])
def test_metrics_specials(device, K):
    torch.manual_seed(K)
    x = torch.randn(6, K, device=device)
    t = torch.randint(0, K, (6,), device=device)
    # row 1: -inf away from the target is an ordinary entry
    x[1, (int(t[1]) + 1) % K] = float("-inf")
    clean, _, _ = _check(x[:3].contiguous(), t[:3].contiguous(), 5)
    ref = loss_sum_fp64(x[:3], t[:3])
    assert abs(float(clean[0]) - ref) <= 2e-6 * abs(ref) + 2e-6 * 3
    # row 3: a NaN (not at the target): incorrect at every k, NaN loss
    x[3, (int(t[3]) + 3) % K] = float("nan")
    nan_row = classification_metrics(x[3:4].contiguous(), t[3:4].contiguous(), k=K).cpu()
    assert nan_row[1:].tolist() == [1.0, 0.0, 0.0] and torch.isnan(nan_row[0])
    # row 4: a target outside [0, K) that is not ignore_index
    t[4] = K + 3
    oor = classification_metrics(x[4:5].contiguous(), t[4:5].contiguous(), k=K).cpu()
    assert oor[1:].tolist() == [1.0, 0.0, 0.0] and torch.isnan(oor[0])
    # all together: counts still exact against the rule
    state, _, _ = _check(x, t, 5)
    assert torch.isnan(state[0])


def _batches(device):
    torch.manual_seed(11)
    out = []
    for B, K in [(64, 10), (37, 10), (130, 10)]:
        out.append((torch.randn(B, K, device=device) * 2, _targets(B, K, device)))
    return out


def test_metrics_accumulate_and_repeat_bitwise(device):
    batches = _batches(device)
    singles = [classification_metrics(x, t, k=5).cpu() for x, t in batches]
    again = [classification_metrics(x, t, k=5).cpu() for x, t in batches]
    assert all(torch.equal(a, b) for a, b in zip(singles, again))
    state = torch.zeros(4, dtype=torch.float64, device=device)
    for x, t in batches:
        out = classification_metrics(x, t, k=5, state=state)
        assert out is state
    host = torch.zeros(4, dtype=torch.float64)
    for s in singles:
        host += s  # the same order of fp64 adds
    assert torch.equal(state.cpu(), host)
    assert state[1:].cpu().tolist() == [float(sum(int(s[i]) for s in singles)) for i in (1, 2, 3)]


def test_metrics_graph_replay_bitwise(device):
    torch.manual_seed(3)
    x = torch.randn(256, 1000, device=device)
    t = _targets(256, 1000, device)
    eager = torch.zeros(4, dtype=torch.float64, device=device)
    for _ in range(3):
        classification_metrics(x, t, k=5, state=eager)  # eager first: allocates counter / scratch
    state = torch.zeros(4, dtype=torch.float64, device=device)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        classification_metrics(x, t, k=5, state=state)
    state.zero_()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(state.cpu(), eager.cpu())
    n, c1, ck = rule_counts(x, t, 5)
    assert state[1:].cpu().tolist() == [3.0 * n, 3.0 * c1, 3.0 * ck]
