"""Time the captured PowerSGD training step with SGD against AdamW in the fused engine and against the
reference-API route to compressed Adam, and the update launches on their own.

    python tools/psgd_adam_bench.py [--configs r18 bert] [--batch 64 512] [--steps 50] [--rounds 6]
                                    [--kernels] [--json-out FILE]

Every arm is its own model + gradient sync + ``StepRunner`` (the engine's runner, graph mode ``auto``),
captured once:

* ``powersgd``        the fused engine with momentum SGD (``psgd_update_wide_kernel``);
* ``powersgd-adamw``  the fused engine with AdamW in its update pass (``psgd_update_adam_wide_kernel``),
                      ``decay_1d=False``, ``weight_decay=0.01``;
* ``powersgd-api``    ``optimizer="adamw"``: the native reducer behind the reference API, then ``FusedAdamW``
                      over the gradients it wrote; the only route to compressed Adam without the arm above.

ResNet-18 runs at rank 4, DistilBERT at rank 8.  A round times ``--steps`` replays of every arm in turn
(host clock around a device sync); the mean over ``--rounds`` is reported with min / max.  ``--kernels``
instead times the update stage alone (HIP events around 200 back-to-back calls of the engines' own
``phase_update`` after one real step, lazy error feedback as the engine runs it) next to ``adamw_step_kernel``
over a flat buffer of the model's parameter count, with the bytes each moves per element: the SGD update
16 B (x, m read and written), the AdamW update 24 B (x, m, v), ``adamw_step`` 28 B (g too).
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
from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync  # noqa: E402
from network_distributed_pytorch_amd.utils.graph import StepRunner  # noqa: E402

ARMS = ("powersgd", "powersgd-adamw", "powersgd-api")
CONFIGS = {"r18": ("resnet18", 4), "bert": ("distilbert", 8)}


def _model(config, device):
    name = CONFIGS[config][0]
    torch.manual_seed(0)
    return build_model(name, 2 if name == "distilbert" else 1000).to(device)


def _sync(name, config, model):
    bert = CONFIGS[config][0] == "distilbert"
    lr, rank = (5e-5 if bert else 1e-3), CONFIGS[config][1]
    if name == "powersgd":
        return build_grad_sync("powersgd", model, lr=lr, momentum=0.9, rank=rank)
    kw = {"optimizer": "adamw"} if name == "powersgd-api" else {}
    sync = build_grad_sync(name, model, lr=lr, momentum=0.9, rank=rank, decay_1d=False, **kw)
    sync.set_hyper(lr, 0.01)
    return sync


def _loss_fn(config, model, batch, device, seq_len):
    if CONFIGS[config][0] == "distilbert":
        from network_distributed_pytorch_amd.utils.data import SyntheticIMDb

        ds = SyntheticIMDb(n=batch, seq_len=seq_len, seed=1234, device=device)
        b = {k: v[:batch].contiguous() for k, v in ds.columns.items()}
        return lambda: model(b["input_ids"], attention_mask=b["attention_mask"], labels=b["labels"])[0]
    crit = CrossEntropyLoss().to(device)
    gen = torch.Generator(device="cpu").manual_seed(1)
    x = (torch.rand(batch, 3, 32, 32, generator=gen) * 2 - 1).to(device)
    y = torch.randint(0, 10, (batch,), generator=gen).to(device)
    return lambda: crit(model(x), y)


class Arm:
    def __init__(self, name, config, batch, device, seq_len):
        self.name = name
        self.model = model = _model(config, device)
        self.sync = _sync(name, config, model)
        loss = _loss_fn(config, model, batch, device, seq_len)

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
            ours = statistics.mean(times["powersgd-adamw"]) if "powersgd-adamw" in times else None
            for arm in arms:
                t = times[arm.name]
                mean = statistics.mean(t)
                block = arm.sync.adam_stats()
                # the reference-API loop keeps no snapshot: its graph warm-up steps count too
                extra = arm.runner.warmup if arm.name == "powersgd-api" and arm.runner.mode != "none" else 0
                assert block is None or block["steps"] == arm.steps + extra, (block, arm.steps)
                arm.sync.check_errors()
                results.append({"config": config, "batch": batch, "rank": CONFIGS[config][1], "arm": arm.name,
                                "ms_per_step_mean": mean, "ms_per_step_min": min(t), "ms_per_step_max": max(t),
                                "delta_to_powersgd_adamw_ms": None if ours is None else mean - ours, "rounds": len(t),
                                "steps_per_round": args.steps, "graph_mode": arm.runner.mode, "adam": block,
                                "parameters": sum(p.numel() for p in arm.model.parameters())})
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
    """The update stage of both engines alone, and adamw_step_kernel over as many elements."""
    results = []
    for config in args.configs:
        bert = CONFIGS[config][0] == "distilbert"
        batch = args.bert_batch if bert else args.batch[0]
        rows = []
        keep = []
        for name, per_elem in (("powersgd", 16), ("powersgd-adamw", 24)):
            model = _model(config, device)
            sync = _sync(name, config, model)
            if sync.overlap:
                sync.set_overlap(False)
            sync.zero_grad()
            _loss_fn(config, model, batch, device, args.seq_len)().backward()
            sync.step()  # one real step: tables bound, P-hat and Q in place
            torch.cuda.synchronize()
            keep.append((model, sync))
            rows.append((f"{name}:phase_update", sync.phase_update, per_elem, sync.arena_numel))
        numel = (keep[0][1].arena_numel + 15) // 16 * 16
        x, g = (torch.randn(numel, device=device) * 1e-2 for _ in range(2))
        adam = ops.FusedAdamW([x], 1e-3, weight_decay=0.01)
        adam.bind([g])
        rows.append(("adamw_step", lambda: adam.step(1.0), 28, numel))
        for _ in range(args.kernel_rounds):
            for name, fn, per_elem, n in rows:
                us = _time(fn)
                results.append({"config": config, "kernel": name, "numel": n, "us": us, "bytes_per_element": per_elem,
                                "bytes_moved": per_elem * n, "tb_per_s": per_elem * n / us / 1e6})
                print(json.dumps(results[-1]), flush=True)
        for _, sync in keep:
            sync.check_errors()
        del keep, rows, x, g, adam
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
    ap.add_argument("--kernels", action="store_true", help="time the update launches alone instead of whole steps")
    ap.add_argument("--kernel-rounds", type=int, default=3)
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("psgd_adam_bench: no HIP device (a timing needs the GPU)")
    assert ops.native_available(), "native extension missing"
    device = torch.device("cuda", 0)
    results = bench_kernels(args, device) if args.kernels else bench_steps(args, device)
    if args.json_out:
        with open(args.json_out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
