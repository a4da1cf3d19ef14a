"""Time captured ResNet-18 training steps with and without a learning-rate schedule / weight decay.

    python tools/hyper_bench.py [--batch 64 512] [--steps 50] [--rounds 7] [--overlap] [--json-out FILE]

Every arm is its own model + PowerSGD sync + ``StepRunner`` (the engine's runner, graph mode
``auto``), captured once; the arms differ only in how the update kernels get their hyper-parameters:

* ``constant``     the default: lr by value, no block, dead-tap compacted plan (the headline path);
* ``block-idle``   ``set_hyper`` before every step with constant values: the kernels read the device
                   block, nothing is ever uploaded;
* ``cosine``       a cosine schedule, no decay: one 16-byte block upload per step, compact plan;
* ``cosine+wd``    cosine and ``weight_decay = 5e-4``: upload per step and the full-layout plan
                   that a decay forces (dead taps need their momentum).

``cosine - block-idle`` is the per-step cost of the upload, ``cosine+wd - cosine`` the cost of the
full layout and of the decay arithmetic.  A round times ``--steps`` replays of every arm in turn
(host clock around a device sync); the median over ``--rounds`` is reported with min / max.
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
from network_distributed_pytorch_amd.utils.schedule import LrSchedule  # noqa: E402

ARMS = ("constant", "block-idle", "cosine", "cosine+wd")
BASE_LR, WD = 0.01, 5e-4


class Arm:
    def __init__(self, name, batch, total_steps, device, num_classes, overlap=None):
        self.name = name
        torch.manual_seed(0)
        self.model = build_model("resnet18", num_classes).to(device)
        crit = CrossEntropyLoss().to(device)
        self.sync = build_grad_sync("powersgd", self.model, lr=BASE_LR, momentum=0.9, rank=4, overlap=overlap)
        gen = torch.Generator(device="cpu").manual_seed(1)
        x = (torch.rand(batch, 3, 32, 32, generator=gen) * 2 - 1).to(device)
        y = torch.randint(0, 10, (batch,), generator=gen).to(device)

        def pre():
            self.sync.zero_grad()
            crit(self.model(x), y).backward()
        self.runner = StepRunner(pre, self.sync, mode="auto", state_tensors=list(self.model.buffers()))
        cosine = name.startswith("cosine")
        self.schedule = LrSchedule(BASE_LR, total_steps, 1, schedule="cosine" if cosine else "constant",
                                   warmup_steps=20 if cosine else 0)
        self.wd = WD if name == "cosine+wd" else 0.0
        self.step = 0
        if name != "constant":
            self.sync.plan_hyper((self.schedule.lr_at(s), self.wd) for s in range(total_steps))

    def run(self, steps):
        for _ in range(steps):
            if self.name != "constant":
                self.sync.set_hyper(self.schedule.lr_at(self.step), self.wd)
            self.runner()
            self.step += 1
        self.runner.join()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 512], help="per-GPU batch size(s)")
    ap.add_argument("--steps", type=int, default=50, help="replays per timed round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10, help="untimed replays after capture")
    ap.add_argument("--num-classes", type=int, default=1000, help="the reference's ResNet head")
    ap.add_argument("--arms", nargs="+", choices=ARMS, default=list(ARMS))
    ap.add_argument("--overlap", action="store_true",
                    help="overlap groups on the side stream: the step is two graphs (compute + comm)")
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("hyper_bench: no HIP device (a timing needs the GPU)")
    assert ops.native_available(), "native extension missing"
    device = torch.device("cuda", 0)
    results = []
    for batch in args.batch:
        total = args.warmup + args.steps * args.rounds
        arms = [Arm(name, batch, total, device, args.num_classes, overlap=True if args.overlap else None)
                for name in args.arms]
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
        for arm in arms:
            t = times[arm.name]
            opt = arm.sync.opt
            arm.sync.check_errors()
            results.append({"batch": batch, "arm": arm.name, "ms_per_step_median": statistics.median(t),
                            "ms_per_step_min": min(t), "ms_per_step_max": max(t), "rounds": len(t),
                            "steps_per_round": args.steps, "graph_mode": arm.runner.mode,
                            "graphs": 1 + len(arm.runner.side_graphs),
                            "block_uploads": opt.hyper.uploads, "steps": arm.step,
                            "compact_matrices": sum(lay is not None for lay in opt.buf.layout),
                            "param_checksum": float(opt.x.double().sum().item())})
            print(json.dumps(results[-1]), flush=True)
        del arms
        torch.cuda.empty_cache()
    if args.json_out:
        with open(args.json_out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
