"""Time the captured dense training step with SGD, AdamW, LARS and LAMB, and the four LAMB / LARS
launches on their own.

    python tools/layerwise_bench.py [--configs r18 bert] [--batch 64 512] [--steps 50] [--rounds 6]
                                    [--kernels] [--json-out FILE]

The arms are those of tools/adamw_bench.py (own model + dense gradient sync + ``StepRunner``, captured
once, timed in alternating rounds) and differ only in the gradient-sync kind: ``dense`` (``sgd``),
``dense`` with ``optimizer="adamw"``, ``dense-lars`` and ``dense-lamb``, the last three with
``decay_1d=False`` and weight decay 0.01.

``--kernels`` times ``lw_norm`` and ``lw_apply`` of both optimisers alone (HIP events around 200
back-to-back launches) over the model's own parameter tensors, one table entry each (the per-tensor
finish depends on how many tensors there are and how large), next to ``adamw_step`` and ``sgd_momentum``
over flat buffers of the same element count, and prints bytes moved per second by the byte model:
LAMB 24 + 16 B per element, LARS 8 + 20, AdamW 28, SGD 20.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import adamw_bench as A  # noqa: E402
from network_distributed_pytorch_amd import ops  # noqa: E402
from network_distributed_pytorch_amd.ops._ext import ext  # noqa: E402
from network_distributed_pytorch_amd.ops.hyper import HyperBlock  # noqa: E402
from network_distributed_pytorch_amd.parallel import trainer  # noqa: E402

ARMS = ("sgd", "adamw", "lars", "lamb")


class Arm(A.Arm):
    """adamw_bench's arm with the gradient-sync kind chosen by the arm's name."""

    def __init__(self, name, config, batch, device, seq_len):
        kind = {"lars": "dense-lars", "lamb": "dense-lamb"}.get(name, "dense")
        build = trainer.build_grad_sync

        def build_kind(_, model, **kw):
            return build(kind, model, **kw, **({"decay_1d": False} if kind != "dense" else {}))
        A.build_grad_sync = build_kind
        try:
            super().__init__(name, config, batch, device, seq_len)
        finally:
            A.build_grad_sync = build
        if kind != "dense":
            self.sync.set_hyper(self.sync.lr, 0.01)


def bench_steps(args, device):
    results = []
    for config in args.configs:
        bert = A.CONFIGS[config] == "distilbert"
        for batch in ([args.bert_batch] if bert else args.batch):
            arms = [Arm(name, config, batch, device, args.seq_len) for name in args.arms]
            for arm in arms:
                arm.run(args.warmup)
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
                trust = getattr(arm.sync, "trust_ratios", lambda: None)()
                results.append({"config": config, "batch": batch, "arm": arm.name, "ms_per_step_mean": statistics.mean(t),
                                "ms_per_step_min": min(t), "ms_per_step_max": max(t), "rounds": len(t),
                                "steps_per_round": args.steps, "graph_mode": arm.runner.mode,
                                "trust_min": None if trust is None else float(trust.min()),
                                "trust_max": None if trust is None else float(trust.max())})
                print(json.dumps(results[-1]), flush=True)
            del arms
            torch.cuda.empty_cache()
    return results


def bench_kernels(args, device):
    results = []
    for config in args.configs:
        params = [p.detach() for p in A._model(config, device).parameters()]
        grads = [torch.randn_like(p) * 1e-2 for p in params]
        mask = [p.dim() > 1 for p in params]
        numel = sum(p.numel() for p in params)
        x, g, buf = (torch.randn((numel + 15) // 16 * 16, device=device) * 1e-2 for _ in range(3))
        hyper = HyperBlock(device, 1e-3, 0.01)
        adam = ops.FusedAdamW([x], 1e-3, weight_decay=0.01)
        adam.bind([g])
        rows = [("adamw_step", lambda: adam.step(1.0), 28),
                ("sgd_momentum", lambda: ops.sgd_momentum_(x, g, buf, 1e-3, 0.9, 1.0, hyper=hyper.dev), 20)]
        for opt, per in ((ops.FusedLamb(params, 1e-3, weight_decay=0.01, adapt_mask=mask), (24, 16)),
                         (ops.FusedLars(params, 1e-3, weight_decay=0.01, adapt_mask=mask), (8, 20))):
            opt.bind(grads)
            opt.step()  # uploads the table
            c = opt.core
            hp = (dict(beta1=c.beta1, beta2=c.beta2, eps=c.eps, mu=0.0, coef=0.0, eps_l=0.0) if c.lamb else
                  dict(beta1=0.0, beta2=0.0, eps=0.0, mu=c.mu, coef=c.coef, eps_l=c.eps_l))
            tab = (c._ent, c._prefix, c._n_ent, c._n_blocks)
            tail = dict(hyper=opt.hyper.dev, m=c.m, v=c.v, block=c.block, div=1.0, **hp)
            rows.append((f"lw_norm_{c.kind}", lambda c=c, tab=tab, tail=tail:
                         ext().lw_norm(c.lamb, *tab, c._partial, c.ctr, c.trust, **tail), per[0]))
            rows.append((f"lw_apply_{c.kind}", lambda c=c, tab=tab, tail=tail:
                         ext().lw_apply(c.lamb, *tab, c.trust, **tail), per[1]))
        for _ in range(args.kernel_rounds):
            for name, fn, per_elem in rows:
                us = A._time(fn)
                results.append({"config": config, "kernel": name, "numel": numel, "tensors": len(params), "us": us,
                                "bytes_per_element": per_elem, "tb_per_s": per_elem * numel / us / 1e6})
                print(json.dumps(results[-1]), flush=True)
        del params, grads, x, g, buf, adam, rows
        torch.cuda.empty_cache()
    return results


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", choices=list(A.CONFIGS), default=list(A.CONFIGS))
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
        raise SystemExit("layerwise_bench: no HIP device (a timing needs the GPU)")
    assert ops.native_available(), "native extension missing"
    device = torch.device("cuda", 0)
    results = bench_kernels(args, device) if args.kernels else bench_steps(args, device)
    if args.json_out:
        with open(args.json_out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
