"""Time captured training steps with and without global-norm gradient clipping, and the two
clipping kernels on their own.

    python tools/clip_bench.py [--configs r18-psgd r18-dense bert-psgd] [--batch 64 512] [--steps 50]
                               [--rounds 6] [--json-out FILE]

Every arm is its own model + gradient sync + ``StepRunner`` (the engine's runner, graph mode
``auto``), captured once; the arms differ only in ``max_grad_norm``:

* ``off``    the default: nothing allocated or launched;
* ``inf``    the norm kernel runs, the scale kernel's workgroups read ``coef == 1`` and return;
* ``clip``   a threshold far below any gradient norm (1e-3): both kernels do their full work
             every step.

``inf - off`` is the cost of the norm pass, ``clip - inf`` that of the scale pass.  A round times
``--steps`` replays of every arm in turn (host clock around a device sync); the mean over
``--rounds`` is reported with min / max.  ``--kernels`` instead times the two launches alone over
a flat buffer of each configuration's gradient size (HIP events around 200 back-to-back pairs) and
reports the norm kernel's read bandwidth.  Its ``clip`` arm uses the threshold 1e-7, below the
rule's ``1e-6`` in the denominator, so that every one of the back-to-back runs scales (with 1e-3 the
buffer reaches norm <= 1e-3 after two runs and the scale kernel returns early from then on).
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
from network_distributed_pytorch_amd.ops.gradclip import GradClip  # noqa: E402
from network_distributed_pytorch_amd.ops.loss import CrossEntropyLoss  # noqa: E402
from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync  # noqa: E402
from network_distributed_pytorch_amd.utils.graph import StepRunner  # noqa: E402

ARMS = {"off": 0.0, "inf": float("inf"), "clip": 1e-3}
# name -> (model, grad sync, PowerSGD rank)
CONFIGS = {"r18-psgd": ("resnet18", "powersgd", 4), "r18-dense": ("resnet18", "dense", 4),
           "bert-psgd": ("distilbert", "powersgd", 8)}


class Arm:
    def __init__(self, name, config, batch, device, seq_len):
        self.name = name
        model_name, kind, rank = CONFIGS[config]
        bert = model_name == "distilbert"
        torch.manual_seed(0)
        self.model = model = build_model(model_name, 2 if bert else 1000).to(device)
        self.sync = build_grad_sync(kind, model, lr=5e-5 if bert else 1e-3, momentum=0.9, rank=rank,
                                    max_grad_norm=ARMS[name])
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
        self.steps = 0

    def run(self, steps):
        for _ in range(steps):
            self.runner()
        self.steps += steps
        self.runner.join()


def bench_steps(args, device):
    results = []
    for config in args.configs:
        bert = CONFIGS[config][0] == "distilbert"
        for batch in ([args.bert_batch] if bert else args.batch):
            arms = [Arm(name, config, batch, device, args.seq_len) for name in args.arms]
            for arm in arms:
                arm.run(args.warmup)
            torch.cuda.synchronize()
            times = {arm.name: [] for arm in arms}
            for _ in range(args.rounds):  # the arms alternate
                for arm in arms:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    arm.run(args.steps)
                    torch.cuda.synchronize()
                    times[arm.name].append(1e3 * (time.perf_counter() - t0) / args.steps)
            off = statistics.mean(times["off"]) if "off" in times else None
            for arm in arms:
                t = times[arm.name]
                if hasattr(arm.sync, "check_errors"):
                    arm.sync.check_errors()
                mean = statistics.mean(t)
                results.append({"config": config, "batch": batch, "arm": arm.name, "ms_per_step_mean": mean,
                                "ms_per_step_min": min(t), "ms_per_step_max": max(t),
                                "delta_to_off_ms": None if off is None else mean - off, "rounds": len(t),
                                "steps_per_round": args.steps, "graph_mode": arm.runner.mode,
                                "clip": arm.sync.clip_stats(), "steps": arm.steps})
                print(json.dumps(results[-1]), flush=True)
            del arms
            torch.cuda.empty_cache()
    return results


def bench_kernels(args, device):
    """The two launches alone over one flat fp32 buffer of each configuration's parameter count."""
    results = []
    for config in args.configs:
        model_name = CONFIGS[config][0]
        numel = sum(p.numel() for p in build_model(model_name, 2 if model_name == "distilbert" else 1000).parameters())
        g = torch.randn(numel, device=device)
        clip = GradClip(device, capacity=1, blocks=(numel + 2047) // 2048)
        clip.bind([g])
        zero = clip.snapshot()
        for name, max_norm in (("inf", float("inf")), ("clip", 1e-7)):
            for _ in range(10):
                clip.run(max_norm)
            reps = 200
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(reps):
                clip.run(max_norm)
            ev[1].record()
            torch.cuda.synchronize()
            us = 1e3 * ev[0].elapsed_time(ev[1]) / reps
            assert clip.read()["clipped"] == (0 if name == "inf" else clip.read()["steps"])
            results.append({"config": config, "numel": numel, "arm": name, "pair_us": us,
                            # norm: one read; scale (clip arm): one read and one write on top
                            "bytes_moved": 4 * numel * (1 if name == "inf" else 3),
                            "gb_per_s": 4 * numel * (1 if name == "inf" else 3) / us / 1e3})
            print(json.dumps(results[-1]), flush=True)
            g.normal_()
            clip.restore(zero)
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
    ap.add_argument("--arms", nargs="+", choices=list(ARMS), default=list(ARMS))
    ap.add_argument("--kernels", action="store_true", help="time the two launches alone instead of whole steps")
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("clip_bench: no HIP device (a timing needs the GPU)")
    assert ops.native_available(), "native extension missing"
    device = torch.device("cuda", 0)
    results = bench_kernels(args, device) if args.kernels else bench_steps(args, device)
    if args.json_out:
        with open(args.json_out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
