"""Time the captured training step with ``grad_sync="signsgd"`` next to ``dense``, ``powersgd`` and
``topk``, and the two scaled-sign launches on their own.

    python tools/signsgd_bench.py [--configs r18 bert] [--batch 64 512] [--steps 50] [--rounds 6]
                                  [--json-out FILE]
    python tools/signsgd_bench.py --kernels [--configs r18 bert] [--world 1]

Every arm is its own model + gradient sync + ``StepRunner`` (the engine's runner, graph mode
``auto``), captured once; the arms differ only in the sync kind.  A round times ``--steps`` replays
of every arm in turn (host clock around a device sync); the mean over ``--rounds`` is reported with
min / max.  One GPU: no collective runs, so the figures are the compute cost of each compressor.

``--kernels`` times the pack and the update launch alone over flat Gaussian arenas with each
configuration's real block table (every parameter at its 16-aligned offset): a repetition runs the
pack and the update in order (the residual feeds the next repetition, as in training) with a HIP
event between the launches; a launch's time is the mean of its event intervals, its bytes are what
the algorithm needs: the pack reads ``g``, ``e`` and writes ``e`` over the live elements plus one
wire buffer, the update reads and writes ``x``, ``b`` and reads ``--world`` wire buffers
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
from network_distributed_pytorch_amd.ops.signsgd import SignCore  # noqa: E402
from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync  # noqa: E402
from network_distributed_pytorch_amd.utils.graph import StepRunner  # noqa: E402

KINDS = ("dense", "powersgd", "topk", "signsgd")
CONFIGS = {"r18": ("resnet18", 4), "bert": ("distilbert", 8)}  # name -> (model, PowerSGD rank)
STAGES = ("pack", "update")


class Arm:
    def __init__(self, kind, config, batch, device, seq_len, label=None, **sync_kw):
        self.kind, self.label = kind, label or kind
        model_name, rank = CONFIGS[config]
        bert = model_name == "distilbert"
        torch.manual_seed(0)
        self.model = model = build_model(model_name, 2 if bert else 1000).to(device)
        self.sync = build_grad_sync(kind, model, lr=5e-5 if bert else 1e-3, momentum=0.9, rank=rank, **sync_kw)
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


def bench_steps(args, device, specs=None):
    """``specs``: ``(label, kind, sync keywords)`` per arm; default: ``args.arms``."""
    specs = specs or [(kind, kind, {}) for kind in args.arms]
    results = []
    for config in args.configs:
        bert = CONFIGS[config][0] == "distilbert"
        for batch in ([args.bert_batch] if bert else args.batch):
            arms = [Arm(kind, config, batch, device, args.seq_len, label, **kw) for label, kind, kw in specs]
            for arm in arms:
                arm.run(args.warmup)
            torch.cuda.synchronize()
            times = {arm.label: [] for arm in arms}
            for _ in range(args.rounds):  # the arms alternate
                for arm in arms:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    arm.run(args.steps)
                    torch.cuda.synchronize()
                    times[arm.label].append(1e3 * (time.perf_counter() - t0) / args.steps)
            for arm in arms:
                t = times[arm.label]
                arm.sync.check_errors()
                results.append({"config": config, "batch": batch, "grad_sync": arm.label,
                                "ms_per_step_mean": statistics.mean(t), "ms_per_step_min": min(t),
                                "ms_per_step_max": max(t), "rounds": len(t), "steps_per_round": args.steps,
                                "graph_mode": arm.runner.mode, "bytes_per_step": arm.sync.bytes_per_step,
                                **({"blocks": arm.sync.core.nb} if arm.kind in ("signsgd", "quant") else {})})
                print(json.dumps(results[-1]), flush=True)
            del arms
            torch.cuda.empty_cache()
    return results


def model_segments(config):
    """``(segments, n, numel)`` of a configuration's parameters laid out as its sync lays them out."""
    model_name = CONFIGS[config][0]
    params = list(build_model(model_name, 2 if model_name == "distilbert" else 1000).parameters())
    segs, n = [], 0
    for p in reversed(params):
        segs.append((n, p.numel()))
        n += (p.numel() + 15) // 16 * 16
    return segs, n, sum(c for _, c in segs)


def time_launches(core, n, world, reps, device):
    """Mean HIP-event interval in us of ``core``'s pack and update launch over Gaussian arenas."""
    g, e, x, b = torch.randn(n, device=device) * 1e-2, torch.zeros(n, device=device), \
        torch.randn(n, device=device), torch.zeros(n, device=device)

    def rep(events=None):
        if events is not None:
            events[0].record()
        out = core.compress(g, e)
        if events is not None:
            events[1].record()
        if world > 1:  # the other ranks' rows: copies of this rank's, outside the timed intervals
            core.gathered.copy_(out.expand(world, -1))
        if events is not None:
            events[2].record()
        core.update(x, b, core.gathered, 1e-3, 0.9)
        if events is not None:
            events[3].record()
    for _ in range(10):
        rep()
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(reps)]
    torch.cuda.synchronize()
    for ev in evs:
        rep(ev)
    torch.cuda.synchronize()
    span = {"pack": (0, 1), "update": (2, 3)}
    return {name: 1e3 * statistics.mean(ev[a].elapsed_time(ev[z]) for ev in evs) for name, (a, z) in span.items()}


def bench_kernels(args, device):
    """The two launches alone over flat fp32 arenas laid out like each configuration's sync lays them out."""
    results = []
    for config in args.configs:
        segs, n, numel = model_segments(config)
        core = SignCore(device, segs, n, args.world)
        us = time_launches(core, n, args.world, args.reps, device)
        wire = 4 * core.words
        need = {"pack": 12 * numel + wire, "update": 16 * numel + args.world * wire}
        for name in STAGES:
            results.append({"config": config, "numel": numel, "n": n, "blocks": core.nb, "world": args.world,
                            "launch": name, "us": us[name], "bytes_needed": need[name],
                            "gb_per_s": need[name] / us[name] / 1e3, "wire_bytes": wire, "reps": args.reps})
            print(json.dumps(results[-1]), flush=True)
    return results


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", choices=list(CONFIGS), default=list(CONFIGS))
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 512], help="ResNet-18 per-GPU batch size(s)")
    ap.add_argument("--bert-batch", type=int, default=16)
    ap.add_argument("--seq-len", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50, help="replays per timed round")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=10, help="untimed replays after capture")
    ap.add_argument("--arms", nargs="+", choices=list(KINDS), default=list(KINDS))
    ap.add_argument("--kernels", action="store_true", help="time the two launches alone instead of whole steps")
    ap.add_argument("--world", type=int, default=1, help="--kernels: rows of the gathered buffer the update reads")
    ap.add_argument("--reps", type=int, default=100, help="--kernels: timed repetitions")
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("signsgd_bench: no HIP device (a timing needs the GPU)")
    assert ops.native_available(), "native extension missing"
    device = torch.device("cuda", 0)
    results = bench_kernels(args, device) if args.kernels else bench_steps(args, device)
    if args.json_out:
        with open(args.json_out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
