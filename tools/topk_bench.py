"""Time the captured training step with ``grad_sync="topk"`` next to ``dense`` and ``powersgd``, and
the top-k launches on their own.

    python tools/topk_bench.py [--configs r18 bert] [--batch 64 512] [--ratio 0.01] [--steps 50]
                               [--rounds 6] [--json-out FILE]
    python tools/topk_bench.py --kernels [--configs r18 bert] [--ratio 0.01]

Every arm is its own model + gradient sync + ``StepRunner`` (the engine's runner, graph mode
``auto``), captured once; the arms differ only in the sync kind.  A round times ``--steps`` replays
of every arm in turn (host clock around a device sync); the mean over ``--rounds`` is reported with
min / max.  One GPU: no collective runs, so the figures are the compute cost of each compressor.

``--kernels`` times the six launches alone over flat Gaussian arenas of each configuration's
parameter count: every repetition runs the five select launches and the update in order (the
residual feeds the next repetition, as in training), with a HIP event between any two launches;
a launch's time is the mean of its event intervals, and its bytes are what the algorithm needs
(``--kernels`` under ``rocprofv3 --kernel-trace --stats`` gives the kernel times without the events).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from network_distributed_pytorch_amd import ops  # noqa: E402
from network_distributed_pytorch_amd.models import build_model  # noqa: E402
from network_distributed_pytorch_amd.ops.loss import CrossEntropyLoss  # noqa: E402
from network_distributed_pytorch_amd.ops.topk import TopKCore, topk_count  # noqa: E402
from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync  # noqa: E402
from network_distributed_pytorch_amd.utils.graph import StepRunner  # noqa: E402

KINDS = ("dense", "powersgd", "topk")
CONFIGS = {"r18": ("resnet18", 4), "bert": ("distilbert", 8)}  # name -> (model, PowerSGD rank)
STAGES = ("pass0", "pass1", "pass2", "count", "compact", "update")


class Arm:
    def __init__(self, kind, config, batch, device, seq_len, ratio):
        self.kind = kind
        model_name, rank = CONFIGS[config]
        bert = model_name == "distilbert"
        torch.manual_seed(0)
        self.model = model = build_model(model_name, 2 if bert else 1000).to(device)
        self.sync = build_grad_sync(kind, model, lr=5e-5 if bert else 1e-3, momentum=0.9, rank=rank,
                                    topk_ratio=ratio)
        if bert:
            from network_distributed_pytorch_amd.utils.data import SyntheticIMDb

            ds = SyntheticIMDb(n=batch, seq_len=seq_len, seed=1234, device=device)
            b = {k: v[:batch].contiguous() for k, v in ds.columns.items()}

            def loss():
                return model(b["input_ids"], attention_mask=b["attention_mask"], labels=b["labels"])[0]
        else:
            crit = CrossEntropyLoss().to(device)
            gen = torch.Generator(device="cpu").manual_seed(1)
            x = (torch.rand(batch, 3, 32, 32, generator=gen) * 2 - 1).to(device)
            y = torch.randint(0, 10, (batch,), generator=gen).to(device)

            def loss():
                return crit(model(x), y)

        def pre():
            self.sync.zero_grad()
            loss().backward()
        self.runner = StepRunner(pre, self.sync, mode="auto", state_tensors=list(model.buffers()))

    def run(self, steps):
        for _ in range(steps):
            self.runner()
        self.runner.join()


def bench_steps(args, device):
    results = []
    for config in args.configs:
        bert = CONFIGS[config][0] == "distilbert"
        for batch in ([args.bert_batch] if bert else args.batch):
            arms = [Arm(kind, config, batch, device, args.seq_len, args.ratio) for kind in args.arms]
            for arm in arms:
                arm.run(args.warmup)
            torch.cuda.synchronize()
            times = {arm.kind: [] for arm in arms}
            for _ in range(args.rounds):  # the arms alternate
                for arm in arms:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    arm.run(args.steps)
                    torch.cuda.synchronize()
                    times[arm.kind].append(1e3 * (time.perf_counter() - t0) / args.steps)
            for arm in arms:
                t = times[arm.kind]
                arm.sync.check_errors()
                results.append({"config": config, "batch": batch, "grad_sync": arm.kind,
                                "ms_per_step_mean": statistics.mean(t), "ms_per_step_min": min(t),
                                "ms_per_step_max": max(t), "rounds": len(t), "steps_per_round": args.steps,
                                "graph_mode": arm.runner.mode, "bytes_per_step": arm.sync.bytes_per_step,
                                **({"topk_ratio": args.ratio, "k": arm.sync.k} if arm.kind == "topk" else {})})
                print(json.dumps(results[-1]), flush=True)
            del arms
            torch.cuda.empty_cache()
    return results


def bench_kernels(args, device):
    """The six launches alone over flat fp32 arenas of each configuration's parameter count."""
    results = []
    for config in args.configs:
        model_name = CONFIGS[config][0]
        numel = sum(p.numel() for p in build_model(model_name, 2 if model_name == "distilbert" else 1000).parameters())
        n = (numel + 15) // 16 * 16
        k = topk_count(numel, args.ratio, n)
        core = TopKCore(device, n, k)
        g, e, x, b = torch.randn(n, device=device) * 1e-2, torch.zeros(n, device=device), \
            torch.randn(n, device=device), torch.zeros(n, device=device)

        def rep(events=None):
            for s in range(6):
                if events is not None:
                    events[s].record()
                if s < 5:
                    core.select(g, e, stage=s)
                else:
                    core.update(x, b, core.gathered, 1e-3, 0.9)
            if events is not None:
                events[6].record()
        for _ in range(10):
            rep()
        evs = [[torch.cuda.Event(enable_timing=True) for _ in range(7)] for _ in range(args.reps)]
        torch.cuda.synchronize()
        for ev in evs:
            rep(ev)
        torch.cuda.synchronize()
        # bytes the algorithm needs: pass 0 reads g, e and writes e; passes 1, 2, count and compact read e
        # (compact also writes 2k words and k zeros); the update reads and writes x, b and reads 2k words
        need = {"pass0": 12 * n, "pass1": 4 * n, "pass2": 4 * n, "count": 4 * n, "compact": 4 * n + 12 * k,
                "update": 16 * n + 8 * k}
        for s, name in enumerate(STAGES):
            us = 1e3 * statistics.mean(ev[s].elapsed_time(ev[s + 1]) for ev in evs)
            results.append({"config": config, "numel": numel, "n": n, "k": k, "launch": name, "us": us,
                            "bytes_needed": need[name], "gb_per_s": need[name] / us / 1e3, "reps": args.reps})
            print(json.dumps(results[-1]), flush=True)
    return results


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", choices=list(CONFIGS), default=list(CONFIGS))
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 512], help="ResNet-18 per-GPU batch size(s)")
    ap.add_argument("--bert-batch", type=int, default=16)
    ap.add_argument("--seq-len", type=int, default=512)
    ap.add_argument("--ratio", type=float, default=0.01, help="topk_ratio")
    ap.add_argument("--steps", type=int, default=50, help="replays per timed round")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=10, help="untimed replays after capture")
    ap.add_argument("--arms", nargs="+", choices=list(KINDS), default=list(KINDS))
    ap.add_argument("--kernels", action="store_true", help="time the six launches alone instead of whole steps")
    ap.add_argument("--reps", type=int, default=100, help="--kernels: timed repetitions")
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("topk_bench: no HIP device (a timing needs the GPU)")
    assert ops.native_available(), "native extension missing"
    device = torch.device("cuda", 0)
    results = bench_kernels(args, device) if args.kernels else bench_steps(args, device)
    if args.json_out:
        with open(args.json_out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
