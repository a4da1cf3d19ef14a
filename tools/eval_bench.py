"""Time a held-out evaluation pass (engine.Evaluator) of ResNet-18 on the device.

    python tools/eval_bench.py [--batch 64 512] [--images 10000] [--passes 5] [--json-out FILE]
    python tools/eval_bench.py --arm native-eager --batch 64 --images 256 --passes 1   # one arm (kernel trace)
    python tools/eval_bench.py --loader-batches 8 --batch 64                            # training-batch loads only

Arms, all over the same synthetic held-out images and the same model:

* ``native-graph``  forward + fused metrics kernel, captured once and replayed per batch;
* ``native-eager``  the same launches issued eagerly;
* ``aten-eager``    eager forward, then the same numbers from ATen ops with a host read per batch
                    (``F.cross_entropy(sum)`` + ``topk`` + ``eq`` + ``any`` + ``sum`` + ``.item()``);
* ``bytes-graph`` / ``bytes-eager``  the native arms over the same images held as bytes
                    (``Uint8ImageDataset``): each batch, its targets and the tail padding are
                    loaded by one ``image_batch_kernel`` launch instead of gathers and copies.  The
                    bytes are the synthetic images through the inverse of the 0.5 / 0.5
                    normalisation, rounded: the same values up to the 8-bit quantisation.

``--loader-batches N`` runs no model: a ``DeviceLoader`` delivers N full training batches into
static tensors, from the fp32 dataset (``--loader fp32``: gather + copy) or the byte dataset
(``--loader bytes``), for a kernel trace of the launches per training batch.

Every pass ends in its host sync (``compute()`` / ``.item()``), so the host clock around a pass is
the pass time.  Passes of the arms alternate; the median over ``--passes`` is reported together
with the spread (min / max).  ``--metrics-only`` times the metric step alone on random logits
with device events.  Launches per batch come from a kernel trace of ``--arm`` runs at two pass
lengths (profiles/eval/).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from network_distributed_pytorch_amd import engine, ops  # noqa: E402
from network_distributed_pytorch_amd.models import build_model  # noqa: E402
from network_distributed_pytorch_amd.ops.metrics import classification_metrics  # noqa: E402
from network_distributed_pytorch_amd.utils.data import (NORMALIZE, DeviceLoader, SyntheticCIFAR10,  # noqa: E402
                                                        Uint8ImageDataset)

ARMS = ("native-graph", "native-eager", "aten-eager", "bytes-graph", "bytes-eager")


def as_bytes(ds):
    """The fp32 images of ``ds`` (in [-1, 1], the 0.5 / 0.5 normalisation) as a byte dataset."""
    mean, std = NORMALIZE["half"]
    x = ds.columns["data"]
    u8 = ((x * 0.5 + 0.5) * 255.0).round_().clamp_(0, 255).to(torch.uint8)
    return Uint8ImageDataset(u8, ds.columns["target"], mean, std)


def aten_metrics(logits, target, k, ignore_index=-100):
    """What a stock evaluation loop does per batch: returns host numbers (one sync)."""
    valid = target != ignore_index
    loss = F.cross_entropy(logits, target, ignore_index=ignore_index, reduction="sum")
    top = logits.topk(k, dim=1).indices
    hit = top.eq(target[:, None])
    c1 = (hit[:, 0] & valid).sum()
    ck = (hit.any(dim=1) & valid).sum()
    return loss.item(), int(valid.sum().item()), int(c1.item()), int(ck.item())


class AtenPass:
    """The evaluator's batching (static padded inputs) with the ATen metric arm."""

    def __init__(self, ev: "engine.Evaluator", k: int):
        self.ev, self.k = ev, k

    def __call__(self):
        ev = self.ev
        t0 = time.perf_counter()
        was = ev.model.training
        ev.model.eval()
        tot = [0.0, 0, 0, 0]
        with torch.no_grad():
            for s in range(0, len(ev.index), ev.batch):
                ev._load(ev.index[s: s + ev.batch])
                out = aten_metrics(ev.model(ev.static["data"]), ev.static_target, self.k)
                tot = [a + b for a, b in zip(tot, out)]
        ev.model.train(was)
        n = tot[1]
        return {"loss": tot[0] / n, "top1": tot[2] / n, "topk": tot[3] / n, "n": n, "k": self.k,
                "eval_s": time.perf_counter() - t0}


def build_arms(model, val, batch, k, device, which):
    arms = {}
    val_u8 = as_bytes(val) if any(n.startswith("bytes") for n in which) else None
    for name in which:
        mode = "full" if name.endswith("-graph") else "none"
        ev = engine.Evaluator(model, val_u8 if name.startswith("bytes") else val, batch=batch, device=device, topk=k,
                              graph_mode=mode)
        arms[name] = AtenPass(ev, k) if name == "aten-eager" else ev
    return arms


def bench_passes(args, device):
    results = []
    val = SyntheticCIFAR10(8, seed=0, device=device, holdout=args.images)[1]
    torch.manual_seed(0)
    model = build_model("resnet18", args.num_classes).to(device)
    which = [args.arm] if args.arm else list(ARMS)
    for batch in args.batch:
        arms = build_arms(model, val, batch, args.topk, device, which)
        recs = {}
        for name, fn in arms.items():  # warm-up: plans, capture, code objects
            for _ in range(args.warmup):
                recs[name] = fn()
        torch.cuda.synchronize()
        times = {name: [] for name in arms}
        for _ in range(args.passes):  # alternate the arms
            for name, fn in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                recs[name] = fn()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
        for name in arms:
            t = times[name]
            r = recs[name]
            results.append({"batch": batch, "arm": name, "images": args.images, "batches": -(-args.images // batch),
                            "pass_ms_median": 1e3 * statistics.median(t), "pass_ms_min": 1e3 * min(t),
                            "pass_ms_max": 1e3 * max(t), "passes": len(t),
                            "loss": r["loss"], "top1": r["top1"], "topk": r["topk"], "n": r["n"]})
            print(json.dumps(results[-1]), flush=True)
    return results


def run_loader(args, device):
    """``--loader-batches`` full training batches delivered into static tensors, nothing else."""
    batch = args.batch[0]
    ds = SyntheticCIFAR10(batch * args.loader_batches, seed=0, device=device)
    if args.loader == "bytes":
        ds = as_bytes(ds)
    loader = DeviceLoader(ds, batch, shuffle=True, seed=0, device=device)
    static = (torch.empty(batch, 3, 32, 32, device=device), torch.empty(batch, dtype=torch.int64, device=device))
    delivered = loader.deliver_into(*static)
    n = 0
    for b in loader:
        if b[0] is not static[0]:  # what the engine does for a dataset that cannot deliver in place
            static[0].copy_(b[0], non_blocking=True)
            static[1].copy_(b[1], non_blocking=True)
        n += 1
    torch.cuda.synchronize()
    rec = {"loader": args.loader, "batch": batch, "batches": n, "delivered_in_place": delivered}
    print(json.dumps(rec), flush=True)
    return [rec]


def bench_metrics_only(args, device):
    """The metric step alone, on random [batch, K] logits: device events around ``iters`` calls.
    The ATen arm includes its per-batch host reads (that is the arm)."""
    results = []
    for batch in args.batch:
        torch.manual_seed(batch)
        x = torch.randn(batch, args.num_classes, device=device)
        t = torch.randint(0, args.num_classes, (batch,), device=device)
        state = torch.zeros(4, dtype=torch.float64, device=device)
        arms = {"native": lambda: classification_metrics(x, t, k=args.topk, state=state),
                "aten": lambda: aten_metrics(x, t, args.topk)}
        for name, fn in arms.items():
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            results.append({"metrics_only": True, "batch": batch, "classes": args.num_classes, "arm": name,
                            "us_per_batch": 1e3 * a.elapsed_time(b) / args.iters, "iters": args.iters})
            print(json.dumps(results[-1]), flush=True)
    return results


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 512], help="per-rank batch size(s)")
    ap.add_argument("--images", type=int, default=10000, help="held-out images per pass")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--topk", type=int, default=5)
    ap.add_argument("--num-classes", type=int, default=1000, help="the reference's ResNet head")
    ap.add_argument("--arm", choices=ARMS, default=None, help="run one arm only (kernel traces)")
    ap.add_argument("--metrics-only", action="store_true")
    ap.add_argument("--loader-batches", type=int, default=0, help="deliver N training batches only (kernel traces)")
    ap.add_argument("--loader", choices=("fp32", "bytes"), default="bytes")
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: no HIP device (a timing needs the GPU)")
    assert ops.native_available(), "native extension missing"
    device = torch.device("cuda", 0)
    if args.loader_batches:
        results = run_loader(args, device)
    else:
        results = bench_metrics_only(args, device) if args.metrics_only else bench_passes(args, device)
    if args.json_out:
        with open(args.json_out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
