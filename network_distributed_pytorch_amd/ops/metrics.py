"""Fused classification metrics on gfx950 (csrc/loss.hip ``cls_metrics_kernel``): held-out loss,
top-1 and top-k accuracy from the logits in ONE launch per batch, accumulated on the device.

The reference's single-GPU script ends on ``model.eval()`` with nothing behind it; the usual
ATen evaluation (``F.cross_entropy`` + ``topk`` + ``eq`` + ``sum`` + ``.item()``) is about eight
launches and a host sync per batch.  Here one kernel of the fused cross-entropy's shape (one
wave per row) adds ``[loss_sum, n_valid, correct1, correctk]`` into an fp64[4] state tensor, so a
whole validation pass needs no host sync until its end and ONE all-reduce.

The rule (identical on device and in the torch fallback), per row whose target is not
``ignore_index``:

* row loss = logsumexp(x) - x[t] in fp32, summed in fp64;
* rank of the target = #{j : x[j] > x[t]} + #{j < t : x[j] == x[t]}; top-1 correct iff
  rank == 0 (= "``torch.argmax``, the first maximum, equals t"), top-k correct iff rank < k:
  ties resolve deterministically towards the lower index;
* a row that holds a NaN, or whose target is outside [0, K), is incorrect at every k and its
  loss is NaN (``ce_fwd`` treats such targets the same way);
* ``pred[b]`` (optional) = index of the first maximum; ignored rows get ``ignore_index``.

CPU tensors and other dtypes run the torch implementation of exactly this rule; fp32 2-D
logits on device require the native kernel (no silent fallback).
"""
from __future__ import annotations

from typing import Any, Dict, Optional

import torch
import torch.distributed as dist

from ._ext import ext

__all__ = ["classification_metrics", "ClassificationMetrics"]

_CTR: dict = {}
_ROWBUF: dict = {}
_RETIRED: list = []  # outgrown row scratch: a captured graph may still hold its address


def _dev_index(device: torch.device) -> int:
    return device.index if device.index is not None else torch.cuda.current_device()


def _counter(device: torch.device) -> torch.Tensor:
    """The kernel's last-workgroup counter, re-armed to 0 by every launch.  One per device and
    NOT the loss kernel's (ops/loss._counter): an eval graph and a training graph never share
    one.  First use is eager (warm-up), never inside a capture."""
    idx = _dev_index(device)
    c = _CTR.get(idx)
    if c is None:
        assert not torch.cuda.is_current_stream_capturing(), "metrics counter must exist before capture"
        c = _CTR[idx] = torch.zeros(1, dtype=torch.int32, device=device)
    return c


def _rowbuf(device: torch.device, rows: int) -> torch.Tensor:
    """Per-row (loss, rank) scratch of one device, grown on eager use only."""
    idx = _dev_index(device)
    buf = _ROWBUF.get(idx)
    if buf is None or buf.numel() < 2 * rows:
        assert not torch.cuda.is_current_stream_capturing(), "metrics row scratch grows during capture"
        if buf is not None:
            _RETIRED.append(buf)
        buf = _ROWBUF[idx] = torch.empty(2 * rows, dtype=torch.float32, device=device)
    return buf


def _torch_metrics(logits: torch.Tensor, target: torch.Tensor, k: int, ignore_index: int, state: torch.Tensor,
                   pred: Optional[torch.Tensor]) -> None:
    """The rule of the module docstring in torch ops (CPU, or dtypes the kernel does not take)."""
    B, K = logits.shape
    x = logits.detach()
    valid = target != ignore_index
    bad = ((target < 0) | (target >= K)) | torch.isnan(x).any(dim=1)
    tc = target.clamp(0, K - 1)
    xt = x.gather(1, tc[:, None])
    below = torch.arange(K, device=x.device)[None, :] < tc[:, None]
    rank = (x > xt).sum(dim=1) + ((x == xt) & below).sum(dim=1)
    rank = torch.where(bad, torch.full_like(rank, K), rank)
    xf = x.float()
    loss = torch.logsumexp(xf, dim=1) - xt[:, 0].float()
    loss = torch.where(bad, torch.full_like(loss, float("nan")), loss)
    upd = torch.stack([loss[valid].double().sum(), valid.sum().double(), (valid & (rank == 0)).sum().double(),
                       (valid & (rank < k)).sum().double()])
    state.add_(upd.to(state.device))
    if pred is not None:
        pred.copy_(torch.where(valid, x.argmax(dim=1), torch.full_like(target, ignore_index)))


def classification_metrics(logits: torch.Tensor, target: torch.Tensor, k: int = 5, ignore_index: int = -100,
                           state: Optional[torch.Tensor] = None,
                           pred: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``state += [loss_sum, n_valid, correct1, correctk]`` over the rows of ``logits`` [B, K]
    whose ``target`` is not ``ignore_index``; returns ``state`` (fp64[4], created zeroed when
    None).  ``pred`` (optional int64[B]) receives the first-maximum index of every row."""
    if logits.dim() != 2 or target.dim() != 1 or target.shape[0] != logits.shape[0]:
        raise ValueError(f"classification_metrics: logits [B, K] and target [B] expected, got "
                         f"{tuple(logits.shape)} / {tuple(target.shape)}")
    B, K = logits.shape
    if not 1 <= int(k) <= K:
        raise ValueError(f"classification_metrics: k must satisfy 1 <= k <= K (k = {k}, K = {K})")
    if B < 1:
        raise ValueError("classification_metrics: empty batch")
    if state is None:
        state = torch.zeros(4, dtype=torch.float64, device=logits.device)
    if state.dtype != torch.float64 or state.numel() != 4:
        raise ValueError("classification_metrics: state must be a float64 tensor of 4 elements")
    if logits.is_cuda and logits.dtype == torch.float32:
        x = logits.detach().contiguous()
        t = target.contiguous()
        ext().cls_metrics(x, t, state, _rowbuf(x.device, B), _counter(x.device), int(ignore_index), int(k), pred)
    else:
        _torch_metrics(logits, target.long(), int(k), int(ignore_index), state, pred)
    return state


def _all_reduce_f64(state: torch.Tensor, comm) -> int:
    """SUM all-reduce of the fp64 state over ``comm``'s ranks, outside its byte accounting
    (the caller reports the bytes); returns the payload bytes.  The native RCCL plane carries
    fp64; the opt-in IPC plane is fp32-only, so there (and on the c10d planes) the reduction
    goes through the c10d group — never downcast."""
    if comm is None or not comm.active:
        return 0
    from ..parallel.comm import IpcDataPlane

    native = comm.native
    if native is not None and state.is_cuda and not isinstance(native, IpcDataPlane):
        native.all_reduce(state, "sum")
    elif state.is_cuda and dist.get_backend(comm.group) != "nccl":
        host = state.cpu()  # gloo reduces host tensors
        dist.all_reduce(host, group=comm.group)
        state.copy_(host)
    else:
        dist.all_reduce(state, group=comm.group)
    return state.numel() * state.element_size()


class ClassificationMetrics:
    """Running held-out loss / top-1 / top-k over any number of batches, accumulated on the
    device: ``update`` launches one kernel and never syncs; ``compute`` is the one host sync.
    ``k`` larger than the class count is clamped for the kernel and reported as ``topk=None``."""

    def __init__(self, k: int = 5, ignore_index: int = -100, device=None):
        if int(k) < 1:
            raise ValueError("ClassificationMetrics: k >= 1 required")
        self.k = int(k)
        self.ignore_index = int(ignore_index)
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self.state = torch.zeros(4, dtype=torch.float64, device=self.device)
        self.num_classes: Optional[int] = None
        self.comm_bytes = 0  # payload of the last compute()'s all-reduce

    def update(self, logits: torch.Tensor, target: torch.Tensor) -> None:
        self.num_classes = int(logits.shape[1])
        classification_metrics(logits, target, k=min(self.k, self.num_classes), ignore_index=self.ignore_index,
                               state=self.state)

    def reset(self) -> None:
        self.state.zero_()

    def compute(self, comm=None) -> Dict[str, Any]:
        total = self.state.clone()
        self.comm_bytes = _all_reduce_f64(total, comm)
        loss_sum, n, c1, ck = (float(v) for v in total.tolist())  # the host sync
        has_k = self.num_classes is None or self.k < self.num_classes
        return {"loss": loss_sum / n if n else float("nan"), "top1": c1 / n if n else float("nan"),
                "topk": (ck / n if n else float("nan")) if has_k else None, "n": int(n), "k": self.k}
