"""Test-side fp64 reference of the soft cross-entropy (ops/loss.py): label smoothing ``eps`` and an
optional second target per row with weight ``1 - lam``, written from the formula, not from
``F.cross_entropy``'s ``label_smoothing``."""
import torch


def soft_ce_fp64(x, ta, eps, tb=None, lam=None, ignore=-100):
    """Mean over the rows with ``ta != ignore`` of
    ``(1 - eps) * (lam * (lse - x[ta]) + (1 - lam) * (lse - x[tb])) + eps * (lse - mean_k x[k])``;
    differentiable in ``x`` (fp64)."""
    valid = ta != ignore
    lse = torch.logsumexp(x, dim=1)
    safe_a = torch.where(valid, ta, torch.zeros_like(ta))
    hard = lse - x.gather(1, safe_a[:, None])[:, 0]
    if tb is not None:
        safe_b = torch.where(valid, tb, torch.zeros_like(tb))
        lam = lam.double()
        hard = lam * hard + (1.0 - lam) * (lse - x.gather(1, safe_b[:, None])[:, 0])
    rows = (1.0 - eps) * hard + eps * (lse - x.mean(dim=1))
    return torch.where(valid, rows, torch.zeros_like(rows)).sum() / valid.sum()


def soft_case(B, K, device, with_b, seed=0):
    """Logits (scaled by 3), targets with every 7th row ignored where ``B > 8``, and with ``with_b`` a
    second target and ``lam`` that include ``ta == tb`` rows and exact 0 and 1."""
    g = torch.Generator().manual_seed(1000 * B + K + seed)
    x = torch.randn(B, K, generator=g) * 3
    ta = torch.randint(0, K, (B,), generator=g)
    tb = lam = None
    if with_b:
        tb = torch.randint(0, K, (B,), generator=g)
        lam = torch.rand(B, generator=g)
        tb[::3] = ta[::3]
        lam[::4] = 1.0
        lam[1::4] = 0.0
    if B > 8:
        ta[::7] = -100
        if with_b:
            tb[::7] = -100
    mv = lambda t: None if t is None else t.to(device)  # noqa: E731
    return x.to(device), ta.to(device), mv(tb), mv(lam)
