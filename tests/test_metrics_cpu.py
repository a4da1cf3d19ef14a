"""Classification metrics without a device: the torch implementation obeys the stated rule
(ties, ignored rows, specials), and the native binding's argument checks raise."""
import math

import pytest
import torch

from network_distributed_pytorch_amd import ops
from network_distributed_pytorch_amd.ops.metrics import ClassificationMetrics, classification_metrics

from .metric_rule import loss_sum_fp64, rule_counts


@pytest.mark.parametrize("B,K,k", [(1, 2, 1), (5, 7, 5), (64, 10, 5), (64, 10, 1), (33, 3, 3), (16, 1500, 5)])
@pytest.mark.parametrize("ties", [False, True])
def test_torch_metrics_obey_rule(B, K, k, ties):
    torch.manual_seed(B + K + k)
    x = torch.randint(-2, 3, (B, K)).float() if ties else torch.randn(B, K) * 3
    t = torch.randint(0, K, (B,))
    if B > 8:
        t[::7] = -100
    pred = torch.empty(B, dtype=torch.int64)
    state = classification_metrics(x, t, k=k, pred=pred)
    n, c1, ck = rule_counts(x, t, k)
    assert state.dtype == torch.float64 and state[1:].tolist() == [float(n), float(c1), float(ck)]
    ref = loss_sum_fp64(x, t)
    assert abs(float(state[0]) - ref) <= 2e-6 * abs(ref) + 2e-6 * n
    assert torch.equal(pred, torch.where(t != -100, x.argmax(dim=1), torch.full_like(t, -100)))


def test_torch_metrics_tie_rule_by_hand():
    # target 2 ties with entries 0 and 3: the earlier one (0) outranks it, the later one does not
    x = torch.tensor([[1.0, 0.0, 1.0, 1.0], [1.0, 0.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0]])
    t = torch.tensor([2, 0, -100])
    s1 = classification_metrics(x, t, k=1)
    assert s1[1:].tolist() == [2.0, 1.0, 1.0]  # only the row whose target is the FIRST maximum
    s2 = classification_metrics(x, t, k=2)
    assert s2[1:].tolist() == [2.0, 1.0, 2.0]  # rank 1 < 2


def test_torch_metrics_specials_and_accumulation():
    x = torch.randn(4, 6)
    t = torch.tensor([1, 2, 3, 9])  # row 3: target out of range
    x[0, 4] = float("-inf")         # ordinary entry
    x[1, 5] = float("nan")          # NaN row: incorrect at every k
    state = classification_metrics(x, t, k=6)
    n, c1, ck = rule_counts(x, t, 6)
    assert (n, ck) == (4, 2) and state[1:].tolist() == [4.0, float(c1), 2.0] and math.isnan(float(state[0]))
    m = ClassificationMetrics(k=5, device="cpu")
    parts = []
    for seed in range(3):
        torch.manual_seed(seed)
        xb, tb = torch.randn(9, 4), torch.randint(0, 4, (9,))
        m.update(xb, tb)
        parts.append(classification_metrics(xb, tb, k=4))
    assert torch.equal(m.state, parts[0] + parts[1] + parts[2])
    rec = m.compute()
    assert rec["n"] == 27 and rec["k"] == 5 and rec["topk"] is None  # k >= K: no top-k figure
    assert rec["loss"] == float(m.state[0]) / 27 and rec["top1"] == float(m.state[2]) / 27
    m.reset()
    assert m.state.tolist() == [0.0] * 4


def test_op_argument_checks():
    x, t = torch.randn(4, 3), torch.randint(0, 3, (4,))
    with pytest.raises(ValueError, match="k must satisfy"):
        classification_metrics(x, t, k=4)
    with pytest.raises(ValueError, match="k must satisfy"):
        classification_metrics(x, t, k=0)
    with pytest.raises(ValueError, match="state"):
        classification_metrics(x, t, k=1, state=torch.zeros(4))


def test_binding_argument_checks():
    """The checks that need no device answer before the device checks do."""
    assert ops.native_available()
    f = ops.ext().cls_metrics
    x, t = torch.randn(4, 3), torch.randint(0, 3, (4,))
    state, rowbuf, ctr = torch.zeros(4, dtype=torch.float64), torch.empty(8), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="k must satisfy 1 <= k <= K"):
        f(x, t, state, rowbuf, ctr, -100, 4)
    with pytest.raises(RuntimeError, match="k must satisfy 1 <= k <= K"):
        f(x, t, state, rowbuf, ctr, -100, 0)
    with pytest.raises(RuntimeError, match="logits must be float32"):
        f(x.double(), t, state, rowbuf, ctr, -100, 1)
    with pytest.raises(RuntimeError, match="target must be contiguous int64"):
        f(x, t.int(), state, rowbuf, ctr, -100, 1)
    with pytest.raises(RuntimeError, match="state must be a contiguous float64"):
        f(x, t, state.float(), rowbuf, ctr, -100, 1)
    with pytest.raises(RuntimeError, match="state must be a contiguous float64"):
        f(x, t, torch.zeros(5, dtype=torch.float64), rowbuf, ctr, -100, 1)
    with pytest.raises(RuntimeError, match="rowbuf"):
        f(x, t, state, torch.empty(7), ctr, -100, 1)
    with pytest.raises(RuntimeError, match="int32 counter"):
        f(x, t, state, rowbuf, ctr.long(), -100, 1)
    with pytest.raises(RuntimeError, match="pred must be contiguous int64"):
        f(x, t, state, rowbuf, ctr, -100, 1, torch.empty(4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="logits must be contiguous"):
        f(x.t().contiguous().t(), t, state, rowbuf, ctr, -100, 1)
    with pytest.raises(RuntimeError, match="empty batch"):
        f(torch.empty(0, 3), torch.empty(0, dtype=torch.int64), state, rowbuf, ctr, -100, 1)
    with pytest.raises(RuntimeError, match="device"):  # everything else in order: host tensors are refused
        f(x, t, state, rowbuf, ctr, -100, 1)
