"""Time the captured training step with ``grad_sync="quant"`` at 2, 4 and 8 bits next to ``dense``,
``powersgd``, ``topk`` and ``signsgd``, and the two block-quantisation launches on their own.

    python tools/quant_bench.py [--configs r18 bert] [--batch 64 512] [--steps 50] [--rounds 6] [--json-out FILE]
    python tools/quant_bench.py --kernels [--configs r18 bert] [--world 1] [--bits 2 4 8]
    python tools/quant_bench.py [--kernels] --bits 4 --rotate none hadamard --arms dense

The method is tools/signsgd_bench.py's (its arms, rounds and event intervals; this tool only adds the
arms).  ``--kernels`` times ``quant_pack`` / ``quant_update`` per bit width and, in the same process
over the same arenas, ``sign_pack`` / ``sign_update`` as the yardstick.  Bytes needed: the pack reads
``g``, ``e`` and writes ``e`` over the live elements plus one row, ``12 + bits / 8`` per element; the
update reads and writes ``x``, ``b`` and reads ``--world`` rows, ``16 + world * bits / 8``.  ``--rotate hadamard``
adds the rotated arms (``quant4rot``: ``quant_rotate="hadamard"``, the ROT kernel instances) beside the plain
ones, in the same process and over the same arenas: the bytes are the same, so the difference is what the
transform costs.
"""
from __future__ import annotations

import argparse
import json

import torch

import signsgd_bench as sb  # the same directory: sys.path[0] of a script

from network_distributed_pytorch_amd import ops  # noqa: E402
from network_distributed_pytorch_amd.ops.quant import QUANT_BITS, QUANT_ROTATIONS, QuantCore  # noqa: E402
from network_distributed_pytorch_amd.ops.signsgd import SignCore  # noqa: E402


_ROT = {"none": "", "hadamard": "rot"}  # the label suffix of an arm


def bench_kernels(args, device):
    results = []
    for config in args.configs:
        segs, n, numel = sb.model_segments(config)
        cores = [("signsgd", SignCore(device, segs, n, args.world))]
        cores += [(f"quant{b}{_ROT[r]}", QuantCore(device, segs, n, args.world, b, rotate=r, rotate_seed=1))
                  for b in args.bits for r in args.rotate]
        for label, core in cores:
            us = sb.time_launches(core, n, args.world, args.reps, device)
            wire = 4 * core.words
            need = {"pack": 12 * numel + wire, "update": 16 * numel + args.world * wire}
            for name in sb.STAGES:
                results.append({"config": config, "core": label, "numel": numel, "blocks": core.nb,
                                "world": args.world, "launch": name, "us": us[name], "bytes_needed": need[name],
                                "gb_per_s": need[name] / us[name] / 1e3, "wire_bytes": wire, "reps": args.reps})
                print(json.dumps(results[-1]), flush=True)
    return results


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", choices=list(sb.CONFIGS), default=list(sb.CONFIGS))
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 512], help="ResNet-18 per-GPU batch size(s)")
    ap.add_argument("--bert-batch", type=int, default=16)
    ap.add_argument("--seq-len", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50, help="replays per timed round")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=10, help="untimed replays after capture")
    ap.add_argument("--arms", nargs="+", choices=list(sb.KINDS), default=list(sb.KINDS), help="the arms beside quant")
    ap.add_argument("--bits", type=int, nargs="+", choices=list(QUANT_BITS), default=list(QUANT_BITS))
    ap.add_argument("--rotate", nargs="+", choices=list(QUANT_ROTATIONS), default=["none"],
                    help="the quant arms' quant_rotate values (hadamard: label suffix 'rot')")
    ap.add_argument("--kernels", action="store_true", help="time the two launches alone instead of whole steps")
    ap.add_argument("--world", type=int, default=1, help="--kernels: rows of the gathered buffer the update reads")
    ap.add_argument("--reps", type=int, default=100, help="--kernels: timed repetitions")
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("quant_bench: no HIP device (a timing needs the GPU)")
    assert ops.native_available(), "native extension missing"
    device = torch.device("cuda", 0)
    if args.kernels:
        results = bench_kernels(args, device)
    else:
        specs = [(k, k, {}) for k in args.arms]
        specs += [(f"quant{b}{_ROT[r]}", "quant", {"quant_bits": b, "quant_rotate": r, "quant_rotate_seed": 1})
                  for b in args.bits for r in args.rotate]
        results = sb.bench_steps(args, device, specs)
    if args.json_out:
        with open(args.json_out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
