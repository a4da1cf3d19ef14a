"""Time the captured dense training step with SGD against AdamW, and the update kernels on their own.

    python tools/adamw_bench.py [--configs r18 bert] [--batch 64 512] [--steps 50] [--rounds 6]
                                [--kernels] [--json-out FILE]

Every arm is its own model + dense gradient sync + ``StepRunner`` (the engine's runner, graph mode
``auto``), captured once; the arms differ only in the optimiser behind the sync:

* ``sgd``    the default: ``sgd_momentum_vec_kernel`` over the flat arena;
* ``adamw``  ``optimizer="adamw"``, ``decay_1d=False`` (the transformer setting): ``adamw_step_kernel``
             over the same arenas plus the second-moment arena.

A round times ``--steps`` replays of every arm in turn (host clock around a device sync); the mean
over ``--rounds`` is reported with min / max.  ``--kernels`` instead times the three streaming
kernels alone (HIP events around 200 back-to-back launches) over flat buffers of the model's
parameter count, and prints bytes moved per second: ``adamw_step`` 28 B per element (g, x, m, v
read; x, m, v written), ``sgd_momentum`` 20 B (g, x, buf read; x, buf written), ``ema_update`` 12 B
(x read, shadow read and written).
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
from network_distributed_pytorch_amd.ops.hyper import HyperBlock  # noqa: E402
from network_distributed_pytorch_amd.ops.loss import CrossEntropyLoss  # noqa: E402
from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync  # noqa: E402
from network_distributed_pytorch_amd.utils.graph import StepRunner  # noqa: E402

ARMS = ("sgd", "adamw")
CONFIGS = {"r18": "resnet18", "bert": "distilbert"}


def _model(config, device):
    name = CONFIGS[config]
    torch.manual_seed(0)
    return build_model(name, 2 if name == "distilbert" else 1000).to(device)


class Arm:
    def __init__(self, name, config, batch, device, seq_len):
        self.name = name
        bert = CONFIGS[config] == "distilbert"
        self.model = model = _model(config, device)
        adam = {"optimizer": "adamw", "decay_1d": False} if name == "adamw" else {}
        self.sync = build_grad_sync("dense", model, lr=5e-5 if bert else 1e-3, momentum=0.9, **adam)
        if name == "adamw":
            self.sync.set_hyper(5e-5 if bert else 1e-3, 0.01)
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
        bert = CONFIGS[config] == "distilbert"
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
            sgd = statistics.mean(times["sgd"]) if "sgd" in times else None
            for arm in arms:
                t = times[arm.name]
                mean = statistics.mean(t)
                block = arm.sync.adam_stats()
                assert block is None or block["steps"] == arm.steps, (block, arm.steps)
                results.append({"config": config, "batch": batch, "arm": arm.name, "ms_per_step_mean": mean,
                                "ms_per_step_min": min(t), "ms_per_step_max": max(t),
                                "delta_to_sgd_ms": None if sgd is None else mean - sgd, "rounds": len(t),
                                "steps_per_round": args.steps, "graph_mode": arm.runner.mode, "adam": block,
                                "arena_elements": arm.sync.ddp.numel,
                                "adam_entries": len(arm.sync.ddp.adam_runs) if block is not None else None})
                print(json.dumps(results[-1]), flush=True)
            del arms
            torch.cuda.empty_cache()
    return results


def _time(fn, reps=200):
    for _ in range(10):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return 1e3 * ev[0].elapsed_time(ev[1]) / reps


def bench_kernels(args, device):
    """The three streaming kernels alone over flat buffers of the model's parameter count."""
    results = []
    for config in args.configs:
        numel = sum(p.numel() for p in _model(config, device).parameters())
        numel = (numel + 15) // 16 * 16
        x, g, buf = (torch.randn(numel, device=device) * 1e-2 for _ in range(3))
        hyper = HyperBlock(device, 1e-3, 0.01)
        adam = ops.FusedAdamW([x], 1e-3, weight_decay=0.01)
        adam.bind([g])
        ema = ops.WeightEma([x], 0.999)
        rows = (("adamw_step", lambda: adam.step(1.0), 28),
                ("sgd_momentum", lambda: ops.sgd_momentum_(x, g, buf, 1e-3, 0.9, 1.0, hyper=hyper.dev), 20),
                ("ema_update", ema.update, 12))
        for _ in range(args.kernel_rounds):
            for name, fn, per_elem in rows:
                us = _time(fn)
                results.append({"config": config, "kernel": name, "numel": numel, "us": us,
                                "bytes_per_element": per_elem, "bytes_moved": per_elem * numel,
                                "tb_per_s": per_elem * numel / us / 1e6})
                print(json.dumps(results[-1]), flush=True)
        assert adam.read()["steps"] == 210 * args.kernel_rounds
        del x, g, buf, adam, ema
        torch.cuda.empty_cache()
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
    ap.add_argument("--kernels", action="store_true", help="time the launches alone instead of whole steps")
    ap.add_argument("--kernel-rounds", type=int, default=3)
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("adamw_bench: no HIP device (a timing needs the GPU)")
    assert ops.native_available(), "native extension missing"
    device = torch.device("cuda", 0)
    results = bench_kernels(args, device) if args.kernels else bench_steps(args, device)
    if args.json_out:
        with open(args.json_out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
