"""The soft cross-entropy front-ends on the CPU (ops/loss.py): the torch composition against the fp64
formula, ``nn.CrossEntropyLoss``'s own label smoothing, the default call and DistilBERT's field."""
import pytest
import torch
import torch.nn.functional as F

from network_distributed_pytorch_amd.ops.loss import CrossEntropyLoss, cross_entropy

from .soft_loss_rule import soft_case, soft_ce_fp64


@pytest.mark.parametrize("B,K", [(1, 7), (16, 2), (33, 10)])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("with_b", [False, True])
def test_composition_matches_fp64_formula(B, K, eps, with_b):
    x, ta, tb, lam = soft_case(B, K, "cpu", with_b)
    if with_b and B > 8:
        assert bool((ta == tb)[ta != -100].any()) and bool((lam == 0).any()) and bool((lam == 1).any())
        assert bool((ta == -100).any())
    x32 = x.clone().requires_grad_(True)
    x64 = x.double().requires_grad_(True)
    loss = cross_entropy(x32, ta, label_smoothing=eps, target_b=tb, lam=lam)
    ref = soft_ce_fp64(x64, ta, eps, tb, lam)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    torch.testing.assert_close(loss.double(), ref, rtol=2e-6, atol=2e-6)
    (loss * 1.7).backward()
    (ref * 1.7).backward()
    torch.testing.assert_close(x32.grad.double(), x64.grad, rtol=1e-5, atol=1e-7)
    if ta.numel() > 8:
        assert float(x32.grad[ta == -100].abs().max()) == 0  # ignored rows: zero gradient


def test_module_honours_label_smoothing_and_targets():
    x, ta, tb, lam = soft_case(33, 10, "cpu", True)
    crit = CrossEntropyLoss(label_smoothing=0.1)
    torch.testing.assert_close(crit(x, ta), F.cross_entropy(x, ta, label_smoothing=0.1))
    torch.testing.assert_close(crit(x, ta, tb, lam).double(), soft_ce_fp64(x.double(), ta, 0.1, tb, lam),
                               rtol=2e-6, atol=2e-6)
    # lam == 1 everywhere is the one-target loss; the default call is F.cross_entropy's
    torch.testing.assert_close(crit(x, ta, tb, torch.ones(33)), crit(x, ta))
    assert torch.equal(CrossEntropyLoss()(x, ta), F.cross_entropy(x, ta))
    acc = torch.zeros(())
    crit.accumulate = acc
    total = crit(x, ta, tb, lam) + crit(x, ta)
    assert torch.equal(acc, total)


def test_front_end_rejects_bad_arguments():
    x, ta, tb, lam = soft_case(16, 5, "cpu", True)
    with pytest.raises(ValueError, match="together"):
        cross_entropy(x, ta, target_b=tb)
    with pytest.raises(ValueError, match="together"):
        cross_entropy(x, ta, lam=lam)
    for eps in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="label_smoothing"):
            cross_entropy(x, ta, label_smoothing=eps)
    with pytest.raises(ValueError, match="reduction"):
        CrossEntropyLoss(reduction="sum")(x, ta, tb, lam)


def test_distilbert_passes_label_smoothing():
    from network_distributed_pytorch_amd.models.distilbert import DistilBertConfig, DistilBertForSequenceClassification

    assert DistilBertConfig().label_smoothing == 0.0
    cfg = DistilBertConfig(vocab_size=50, max_position_embeddings=8, dim=16, n_layers=1, n_heads=2, hidden_dim=32,
                           dropout=0.0, attention_dropout=0.0, seq_classif_dropout=0.0)
    torch.manual_seed(0)
    model = DistilBertForSequenceClassification(cfg).eval()
    ids = torch.randint(1, 50, (4, 8))
    labels = torch.tensor([0, 1, 1, 0])
    plain, logits = model(ids, attention_mask=torch.ones_like(ids), labels=labels)
    torch.testing.assert_close(plain, F.cross_entropy(logits, labels))
    model.config.label_smoothing = 0.1
    smooth, logits2 = model(ids, attention_mask=torch.ones_like(ids), labels=labels)
    assert torch.equal(logits, logits2)
    torch.testing.assert_close(smooth, F.cross_entropy(logits, labels, label_smoothing=0.1))
    assert float(smooth.detach()) != float(plain.detach())
