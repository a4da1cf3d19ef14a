"""Time captured training steps with and without the weight EMA, the two EMA kernels on their own,
and a held-out pass on both weight sets.

    python tools/ema_bench.py [--configs r18-psgd r18-dense bert-psgd] [--batch 64 512] [--steps 50]
                              [--rounds 6] [--overlap] [--kernels | --eval] [--json-out FILE]

Every arm is its own model + gradient sync + ``StepRunner`` (the engine's runner, graph mode
``auto``), captured once; the arms differ only in the attached EMA:

* ``off``   the default: nothing allocated or launched;
* ``ema``   ``ops.WeightEma`` (decay 0.999, warm-up) over the engine's targets (every parameter and
            every persistent fp32 buffer), attached to the sync: one launch behind the step's last
            update launch.

A round times ``--steps`` replays of every arm in turn (host clock around a device sync); the mean
over ``--rounds`` is reported with min / max.  ``--overlap`` builds the PowerSGD arms with overlap
groups: the step is two graphs and the EMA launch is the comm graph's last item, ahead of the
release of the next compute graph.  ``--kernels`` instead times ``ema_update`` / ``ema_swap`` alone
(HIP events around 200 back-to-back launches) over the model's own table and over one flat buffer of
the same size, next to ``grad_sqnorm`` + early-exit ``grad_scale`` over that buffer (the rate
profiles/clip reports), and prints bytes moved per second: 12 B per element for the update (x read,
s read and written), 16 B for the swap.  ``--eval`` times a held-out pass of ResNet-18 on the live
weights alone and on both weight sets (two passes and two swaps).
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

from network_distributed_pytorch_amd import engine, ops  # noqa: E402
from network_distributed_pytorch_amd.models import build_model  # noqa: E402
from network_distributed_pytorch_amd.ops.gradclip import GradClip  # noqa: E402
from network_distributed_pytorch_amd.ops.loss import CrossEntropyLoss  # noqa: E402
from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync  # noqa: E402
from network_distributed_pytorch_amd.utils.graph import StepRunner  # noqa: E402

ARMS = {"off": 0.0, "ema": 0.999}
# name -> (model, grad sync, PowerSGD rank)
CONFIGS = {"r18-psgd": ("resnet18", "powersgd", 4), "r18-dense": ("resnet18", "dense", 4),
           "bert-psgd": ("distilbert", "powersgd", 8)}


def _model(config, device):
    model_name = CONFIGS[config][0]
    torch.manual_seed(0)
    return build_model(model_name, 2 if model_name == "distilbert" else 1000).to(device)


class Arm:
    def __init__(self, name, config, batch, device, seq_len, overlap):
        self.name = name
        model_name, kind, rank = CONFIGS[config]
        bert = model_name == "distilbert"
        self.model = model = _model(config, device)
        kw = {"overlap": True, "groups": 2} if overlap and kind == "powersgd" else {}
        self.sync = build_grad_sync(kind, model, lr=5e-5 if bert else 1e-3, momentum=0.9, rank=rank, **kw)
        self.ema = None
        if ARMS[name]:
            self.ema = ops.WeightEma(engine.ema_targets(model)[1], ARMS[name])
            self.sync.attach_ema(self.ema)
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
            arms = [Arm(name, config, batch, device, args.seq_len, args.overlap) for name in args.arms]
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
                block = arm.ema.read() if arm.ema is not None else None
                assert block is None or block["updates"] == arm.steps, (block, arm.steps)
                results.append({"config": config, "batch": batch, "arm": arm.name, "overlap": bool(args.overlap),
                                "ms_per_step_mean": mean, "ms_per_step_min": min(t), "ms_per_step_max": max(t),
                                "delta_to_off_ms": None if off is None else mean - off, "rounds": len(t),
                                "steps_per_round": args.steps, "graph_mode": arm.runner.mode,
                                "graphs": 1 + len(arm.runner.side_graphs), "ema": block, "steps": arm.steps,
                                "ema_elements": None if arm.ema is None else sum(s.numel() for s in arm.ema.shadow),
                                "ema_entries": None if arm.ema is None else arm.ema.plan.table()[2]})
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
    """The launches alone: the model's own table, and one flat buffer of the same element count."""
    results = []
    for config in args.configs:
        model = _model(config, device)
        sync = build_grad_sync(CONFIGS[config][1], model, lr=1e-3, momentum=0.9, rank=CONFIGS[config][2])
        targets = engine.ema_targets(model)[1]
        numel = sum(t.numel() for t in targets)
        flat = torch.randn(numel, device=device)
        for table, tensors in (("model", targets), ("flat", [flat])):
            ema = ops.WeightEma(tensors, 0.999)
            for t in tensors:  # x != s, as in training
                t.add_(1e-3)
            for name, fn, per_elem in (("ema_update", ema.update, 12), ("ema_swap", ema.swap, 16)):
                us = _time(fn)
                results.append({"config": config, "table": table, "kernel": name, "numel": numel,
                                "entries": ema.plan.table()[2], "blocks": ema.plan.table()[3], "us": us,
                                "bytes_moved": per_elem * numel, "gb_per_s": per_elem * numel / us / 1e3})
                print(json.dumps(results[-1]), flush=True)
            assert ema.read()["updates"] == 210
        clip = GradClip(device, capacity=1, blocks=(numel + 2047) // 2048)
        clip.bind([flat])
        us = _time(lambda: clip.run(float("inf")))
        results.append({"config": config, "table": "flat", "kernel": "grad_sqnorm + early-exit grad_scale",
                        "numel": numel, "us": us, "bytes_moved": 4 * numel, "gb_per_s": 4 * numel / us / 1e3})
        print(json.dumps(results[-1]), flush=True)
        del sync, model, flat
        torch.cuda.empty_cache()
    return results


def bench_eval(args, device):
    """A held-out pass of ResNet-18 (synthetic CIFAR, graph replays) on the live weights alone and on
    both weight sets: two passes and two swap launches, the same evaluator."""
    from network_distributed_pytorch_amd.utils.data import SyntheticCIFAR10

    results = []
    for batch in args.batch:
        model = _model("r18-psgd", device)
        _, val = SyntheticCIFAR10(n=batch, seed=1234, device=device, holdout=args.eval_size)
        ev = engine.Evaluator(model, val, batch=batch, device=device, graph_mode="auto")
        ema = ops.WeightEma(engine.ema_targets(model)[1], 0.999)

        def single():
            return ev()

        def both():
            rec = ev()
            ema.swap()
            try:
                ev()
            finally:
                ema.swap()
            return rec
        single()  # warm-up batch + capture
        times = {"single": [], "both": []}
        for _ in range(args.rounds):
            for name, fn in (("single", single), ("both", both)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append(1e3 * (time.perf_counter() - t0))
        swap_us = _time(ema.swap)
        for name, t in times.items():
            results.append({"eval": name, "batch": batch, "eval_size": args.eval_size, "ms_mean": statistics.mean(t),
                            "ms_min": min(t), "ms_max": max(t), "rounds": len(t), "swap_us": swap_us,
                            "replays": ev.replays})
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
    ap.add_argument("--arms", nargs="+", choices=list(ARMS), default=list(ARMS))
    ap.add_argument("--overlap", action="store_true", help="PowerSGD arms with overlap groups (two graphs per step)")
    ap.add_argument("--kernels", action="store_true", help="time the launches alone instead of whole steps")
    ap.add_argument("--eval", action="store_true", help="time a held-out pass on one and on both weight sets")
    ap.add_argument("--eval-size", type=int, default=10000)
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("ema_bench: no HIP device (a timing needs the GPU)")
    assert ops.native_available(), "native extension missing"
    device = torch.device("cuda", 0)
    if args.kernels:
        results = bench_kernels(args, device)
    elif args.eval:
        results = bench_eval(args, device)
    else:
        results = bench_steps(args, device)
    if args.json_out:
        with open(args.json_out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
