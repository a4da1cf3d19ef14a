"""Time the ResNet-18 training step on byte images with and without label smoothing and mixup /
CutMix, and the two new kernels against the ones they stand in for.

    python tools/mix_bench.py [--batch 64 512] [--steps 50] [--rounds 6] [--json-out FILE]
    python tools/mix_bench.py --kernels [--batch 64 512] [--reps 200]

Every arm is its own model + PowerSGD sync + ``StepRunner`` (the engine's runner, graph mode
``auto``), captured once, fed the engine's way: per step one batch launch of ``Uint8ImageDataset``
writes the captured step's static inputs in place, then the graph is replayed.  The arms differ only
in the regularisers:

* ``off``     the default: ``image_batch_kernel`` and ``ce_fwd_kernel``;
* ``smooth``  ``label_smoothing=0.1``: ``ce_soft_fwd_kernel`` with one target;
* ``mix``     ``mix="mixup_cutmix"``: ``image_mix_batch_kernel`` and ``ce_soft_fwd_kernel`` with two;
* ``both``    the two together.

A round times ``--steps`` steps of every arm in turn (host clock around a device sync); the mean
over ``--rounds`` is reported with min / max and the difference to ``off``.  ``--kernels`` instead
launches each of the four kernels ``--reps`` times back to back between HIP events, at the same
batch sizes (1000 classes for the loss, as the step has): the per-launch time includes the launch
gap, so run it under a kernel trace for the kernels' own durations.
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
from network_distributed_pytorch_amd.ops.loss import CrossEntropyLoss, cross_entropy  # noqa: E402
from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync  # noqa: E402
from network_distributed_pytorch_amd.utils.data import NORMALIZE, Uint8ImageDataset  # noqa: E402
from network_distributed_pytorch_amd.utils.graph import StepRunner  # noqa: E402

# name -> (label_smoothing, mix)
ARMS = {"off": (0.0, "none"), "smooth": (0.1, "none"), "mix": (0.0, "mixup_cutmix"), "both": (0.1, "mixup_cutmix")}
N_IMAGES = 8192


def _dataset(device, mix="none"):
    g = torch.Generator(device="cpu").manual_seed(1)
    images = torch.randint(0, 256, (N_IMAGES, 3, 32, 32), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (N_IMAGES,), generator=g)
    mean, std = NORMALIZE["cifar"]
    return Uint8ImageDataset(images, labels, mean, std, pad=4, flip=True, mix=mix, mix_prob=1.0).to(device)


class Arm:
    def __init__(self, name, batch, device):
        self.name = name
        eps, mix = ARMS[name]
        torch.manual_seed(0)
        self.model = model = build_model("resnet18", 1000).to(device)
        self.sync = build_grad_sync("powersgd", model, lr=1e-3, momentum=0.9, rank=4)
        self.ds = _dataset(device, mix)
        crit = CrossEntropyLoss(label_smoothing=eps).to(device)
        self.static = [torch.zeros(batch, 3, 32, 32, device=device),
                       torch.zeros(batch, dtype=torch.int64, device=device)]
        if mix != "none":
            self.static += [torch.zeros(batch, dtype=torch.int64, device=device), torch.ones(batch, device=device)]
        order = torch.randperm(N_IMAGES, generator=torch.Generator(device="cpu").manual_seed(2))
        self.batches = [order[s: s + batch].to(device) for s in range(0, N_IMAGES - batch + 1, batch)]
        static = self.static

        def pre():
            self.sync.zero_grad()
            crit(model(static[0]), *static[1:]).backward()
        self.load(0)
        self.runner = StepRunner(pre, self.sync, mode="auto", state_tensors=list(model.buffers()))
        self.steps = 0

    def load(self, step):
        self.ds.gather_into(self.batches[step % len(self.batches)], *self.static, pad_target=-100,
                            epoch=step // len(self.batches), seed=714, augment=True)

    def run(self, steps):
        for _ in range(steps):
            self.load(self.steps)
            self.runner()
            self.steps += 1
        self.runner.join()


def bench_steps(args, device):
    results = []
    for batch in args.batch:
        arms = [Arm(name, batch, device) for name in args.arms]
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
            arm.ds.check_errors()
            mean = statistics.mean(t)
            results.append({"batch": batch, "arm": arm.name, "ms_per_step_mean": mean, "ms_per_step_min": min(t),
                            "ms_per_step_max": max(t), "delta_to_off_ms": None if off is None else mean - off,
                            "ratio_to_off": None if off is None else mean / off, "rounds": len(t),
                            "steps_per_round": args.steps, "graph_mode": arm.runner.mode, "steps": arm.steps})
            print(json.dumps(results[-1]), flush=True)
        del arms
        torch.cuda.empty_cache()
    return results


def _time(fn, reps):
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
    """Each kernel alone, back to back: the batch launch at ``mix_prob = 1`` (every row but the centre
    one reads its partner), the loss forward at 1000 classes."""
    results = []
    for batch in args.batch:
        plain, mixed = _dataset(device), _dataset(device, "mixup_cutmix")
        idx = torch.randperm(N_IMAGES, generator=torch.Generator(device="cpu").manual_seed(3))[:batch].to(device)
        out = torch.zeros(batch, 3, 32, 32, device=device)
        tgt = torch.zeros(batch, dtype=torch.int64, device=device)
        tgt_b, lam = torch.zeros_like(tgt), torch.ones(batch, device=device)
        x = torch.randn(batch, 1000, device=device)
        kw = dict(pad_target=-100, epoch=1, seed=714, augment=True)
        mixed.gather_into(idx, out, tgt, tgt_b, lam, **kw)
        cases = {
            "image_batch_kernel": lambda: plain.gather_into(idx, out, tgt, **kw),
            "image_mix_batch_kernel": lambda: mixed.gather_into(idx, out, tgt, tgt_b, lam, **kw),
            "ce_fwd_kernel": lambda: cross_entropy(x, tgt),
            "ce_soft_fwd_kernel": lambda: cross_entropy(x, tgt, label_smoothing=0.1, target_b=tgt_b, lam=lam),
        }
        us = {name: _time(fn, args.reps) for name, fn in cases.items()}
        for name, base in (("image_batch_kernel", None), ("image_mix_batch_kernel", "image_batch_kernel"),
                           ("ce_fwd_kernel", None), ("ce_soft_fwd_kernel", "ce_fwd_kernel")):
            results.append({"batch": batch, "kernel": name, "us_per_call": us[name], "reps": args.reps,
                            "ratio_to_plain": None if base is None else us[name] / us[base]})
            print(json.dumps(results[-1]), flush=True)
    return results


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 512], help="per-GPU batch size(s)")
    ap.add_argument("--steps", type=int, default=50, help="steps per timed round")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=10, help="untimed steps after capture")
    ap.add_argument("--arms", nargs="+", choices=list(ARMS), default=list(ARMS))
    ap.add_argument("--kernels", action="store_true", help="time the four launches alone instead of whole steps")
    ap.add_argument("--reps", type=int, default=200, help="--kernels: back-to-back calls per timing")
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mix_bench: no HIP device (a timing needs the GPU)")
    assert ops.native_available(), "native extension missing"
    device = torch.device("cuda", 0)
    results = bench_kernels(args, device) if args.kernels else bench_steps(args, device)
    if args.json_out:
        with open(args.json_out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
