"""CPU reference of the classification-metric rule (ops/metrics.py), written row by row and
independent of the op's own torch implementation: shared by the metric and evaluation tests."""
import math

import torch
import torch.nn.functional as F


def rule_counts(logits: torch.Tensor, target: torch.Tensor, k: int, ignore_index: int = -100):
    """(n_valid, correct1, correctk) of the stated rule on the given fp32 logits:
    rank = #{j : x[j] > x[t]} + #{j < t : x[j] == x[t]}; a NaN row or an out-of-range target is
    incorrect at every k."""
    x = logits.detach().cpu()
    t = target.detach().cpu().tolist()
    K = x.shape[1]
    n = c1 = ck = 0
    for b, tb in enumerate(t):
        if tb == ignore_index:
            continue
        n += 1
        row = x[b]
        if not 0 <= tb < K or bool(torch.isnan(row).any()):
            continue
        xt = row[tb]
        rank = int((row > xt).sum()) + int((row[:tb] == xt).sum())
        c1 += rank == 0
        ck += rank < k
    return n, c1, ck


def loss_sum_fp64(logits: torch.Tensor, target: torch.Tensor, ignore_index: int = -100) -> float:
    return float(F.cross_entropy(logits.detach().cpu().double(), target.detach().cpu(), ignore_index=ignore_index,
                                 reduction="sum"))


def rule_record(logits: torch.Tensor, target: torch.Tensor, k: int, ignore_index: int = -100):
    """{"n", "top1", "topk", "loss"} as evaluation reports them (loss = fp64 reference mean)."""
    n, c1, ck = rule_counts(logits, target, min(k, logits.shape[1]), ignore_index)
    return {"n": n, "top1": c1 / n if n else math.nan, "topk": ck / n if k < logits.shape[1] else None,
            "loss": loss_sum_fp64(logits, target, ignore_index) / n if n else math.nan}
