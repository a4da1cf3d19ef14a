"""AdamW in the flat-arena compressors on the device (``topk-adamw``, ``signsgd-adamw``, ``quant-adamw``):
the three update launches against the CPU twin, bitwise, and against a plain fp64 evaluation of the
rule; the syncs against the CPU syncs and a captured step against the eager ones."""
import math

import pytest
import torch

from network_distributed_pytorch_amd.models.mlp import ToyMLP
from network_distributed_pytorch_amd.ops.adamw import AdamState
from network_distributed_pytorch_amd.ops.quant import QuantCore, quant_word_shift
from network_distributed_pytorch_amd.ops.signsgd import SignCore, sign_word_bit
from network_distributed_pytorch_amd.ops.topk import TopKCore
from network_distributed_pytorch_amd.parallel.comm import Communicator
from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync

from .test_signsgd_gpu import _bits, _grads

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U = 2.0 ** -24
NUMELS, DIMS = (3, 2048, 2049, 17, 4100), (1, 2, 1, 2, 1)  # each padded to 16: a flag boundary inside a
OFFS = (0, 16, 2064, 4128, 4160)                            # top-k tile and next to ragged blocks
N_ARENA = 8272
LR, BETA1, BETA2, EPS = 0.01, 0.9, 0.95, 1e-8
ARMS = ("signsgd", "quant2", "quant4", "quant8", "topk")


def _core(arm, device, world):
    segs = list(zip(OFFS, NUMELS))
    if arm == "topk":
        return TopKCore(device, N_ARENA, 37, world)
    return SignCore(device, segs, N_ARENA, world) if arm == "signsgd" else QuantCore(device, segs, N_ARENA, world,
                                                                                    int(arm[5:]))


def _decays(core, arm, decay_1d):
    flags = [decay_1d or d > 1 for d in DIMS]
    return core.decay_runs(list(zip(OFFS, flags))) if arm == "topk" else core.block_decays(flags)


def _wire(arm, N, gen):
    """``[N, words]``: one rank's compressed Gaussian gradient per row (the existing CPU compress / select)."""
    one, rows = _core(arm, "cpu", 1), []
    live = torch.zeros(N_ARENA)
    for o, c in zip(OFFS, NUMELS):
        live[o: o + c] = 1.0
    for _ in range(N):
        g, e = torch.randn(N_ARENA, generator=gen) * live, torch.zeros(N_ARENA)
        rows.append((one.select(g, e) if arm == "topk" else one.compress(g, e)).clone())
    return torch.stack(rows)


def _plain_o(arm, core, rows):
    """(sum of the decoded values / N, sum of their magnitudes / N) per arena element, in fp64, decoded
    element by element from the documented wire layout; elements outside every block hold 0."""
    N = rows.shape[0]
    o, mag = torch.zeros(N_ARENA, dtype=torch.float64), torch.zeros(N_ARENA, dtype=torch.float64)
    for r in range(N):
        row = rows[r]
        if arm == "topk":
            idx, val = row[: core.k].long(), row[core.k:].view(torch.float32).double()
            o[idx] += val
            mag[idx] += val.abs()
            continue
        for j, (off, ln) in enumerate(core._host_table.tolist()):
            t = torch.arange(ln)
            if arm == "signsgd":
                w, b = sign_word_bit(j, t)
                s = (row[core.nb * 64 + j] & 0x7FFFFFFF).view(torch.float32).double()
                c = torch.where(((row[w] >> b) & 1) == 1, -s, s)
            else:
                w, sh = quant_word_shift(core.bits, j, t)
                u = (row[w] >> sh.to(torch.int32)) & (2 ** core.bits - 1)
                c = (u - core.levels).double() * row[core.code_words + j].view(torch.float32).double()
            o[off: off + ln] += c
            mag[off: off + ln] += c.abs()
    return o / N, mag / N


@pytest.mark.parametrize("decay_1d", [True, False])
@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("arm", ARMS)
def test_update_adam_is_the_twin_bitwise_and_the_fp64_rule_within_rounding(arm, N, wd, decay_1d):
    """Three launches (block steps 1, 2, 3).  The bound per element is ``K 2^-24`` times the sum of the
    magnitudes of the addends of the quantity's last operation, ``K`` the number of correctly rounded
    fp32 operations that feed it (each at most ``2^-24`` relative to its result, first order):

    * ``o``: a product per rank (quant), ``N`` adds, one division: ``K_o = 2 N + 1``; its addends are
      the ranks' values, so ``|o|`` enters every bound as ``mag = sum |c_r| / N``.
    * ``m' = b1 m + om1 o``: ``om1``, two products, the add: ``K_m = 4 + K_o`` over ``|b1 m| + om1 mag``.
    * ``v' = b2 v + om2 o^2``: ``om2``, three products, the add, ``o`` twice: ``K_v = 5 + 2 K_o`` over
      ``b2 v + om2 mag^2``.
    * ``x' = x1 - u``, ``u = ss (m' / den)``: ``x1`` 3 (``lr wd``, ``1 - .``, the product), the
      subtraction 1, ``ss = lr / (1 - p1)`` ``2 + A1`` (the error of ``p1`` is amplified by
      ``A1 = p1 / (1 - p1)``), product and quotient 2, ``m'`` ``K_m``, ``den = sqrt(v') / sb + eps``
      ``K_v / 2 + 1 + ((A2 + 1) / 2 + 1) + 2`` with ``A2 = p2 / (1 - p2)``; over ``|x1| + |u|``.
      ``A1``, ``A2`` at step 3, where they are largest.
    """
    gen = torch.Generator().manual_seed(1000 * N + len(arm))
    cpu, dev = _core(arm, "cpu", N), _core(arm, DEV, N)
    blk_c, blk_d = AdamState("cpu", cpu.adam_grid), AdamState(DEV, dev.adam_grid)
    dec_c, dec_d = _decays(cpu, arm, decay_1d), _decays(dev, arm, decay_1d)
    hyper = torch.tensor([LR, wd, 0.0, 0.0], device=DEV)
    lr32, wd32, b1, b2 = (float(torch.tensor(v, dtype=torch.float32)) for v in (LR, wd, BETA1, BETA2))
    decays, live = (torch.zeros(N_ARENA, dtype=torch.bool) for _ in range(2))
    for o, c, d in zip(OFFS, NUMELS, DIMS):
        live[o: o + c], decays[o: o + c] = True, (decay_1d or d > 1) and wd != 0
    x = torch.randn(N_ARENA, generator=gen)
    x[~live] = 0.0 if arm == "topk" else 12345.0  # zero padding stays zero; outside every block nothing is touched
    m, v = torch.zeros(N_ARENA), torch.zeros(N_ARENA)
    xd, md, vd = (t.clone().to(DEV) for t in (x, m, v))
    A1, A2, Ko = b1 ** 3 / (1 - b1 ** 3), b2 ** 3 / (1 - b2 ** 3), 2 * N + 1
    Km, Kv = 4 + Ko, 5 + 2 * Ko
    Kx = math.ceil(3 + 1 + (2 + A1) + 2 + Km + (Kv / 2 + 1 + ((A2 + 1) / 2 + 1) + 2))
    for step in range(1, 4):
        rows = _wire(arm, N, gen)
        st = blk_c.read()
        x0, m0, v0 = x.double(), m.double(), v.double()
        cpu.update_adam(x, m, v, rows, LR, wd, BETA1, BETA2, EPS, blk_c, dec_c)
        dev.update_adam(xd, md, vd, rows.to(DEV), LR, wd, BETA1, BETA2, EPS, blk_d, dec_d, hyper)
        for a, b in ((xd, x), (md, m), (vd, v)):
            assert torch.equal(_bits(a), _bits(b)), (step, (a.cpu() != b).sum())
        assert blk_d.read() == blk_c.read() and blk_c.read()["steps"] == step
        o, mag = _plain_o(arm, cpu, rows)
        p1, p2 = st["b1pow"] * b1, st["b2pow"] * b2
        x1 = torch.where(decays, x0 * (1 - lr32 * wd32), x0)
        m1, v1 = b1 * m0 + (1 - b1) * o, b2 * v0 + (1 - b2) * o * o
        u = lr32 / (1 - p1) * (m1 / (v1.sqrt() / math.sqrt(1 - p2) + float(torch.tensor(EPS, dtype=torch.float32))))
        errs = {"x": ((x.double() - (x1 - u)).abs(), Kx * U * (x1.abs() + u.abs())),
                "m": ((m.double() - m1).abs(), Km * U * ((b1 * m0).abs() + (1 - b1) * mag)),
                "v": ((v.double() - v1).abs(), Kv * U * (b2 * v0 + (1 - b2) * mag * mag))}
        for name, (err, bound) in errs.items():
            worst = (err / bound.clamp_min(1e-300))[live].max().item()
            print(f"{arm} N={N} wd={wd} decay_1d={decay_1d} step {step} {name}: worst err / bound = {worst:.3f}")
            assert (err <= bound)[live].all(), (name, step, worst)
        assert torch.equal(_bits(x)[~live], _bits(x0.float())[~live]) and not m[~live].any() and not v[~live].any()


def _sync(device, kind):
    torch.manual_seed(0)
    model = ToyMLP().to(device)
    return model, build_grad_sync(kind, model, Communicator(), lr=0.01, decay_1d=False, betas=(BETA1, BETA2),
                                  quant_bits=4, topk_ratio=0.05)


def _state(sync):
    return [_bits(t) for t in (sync.x, sync.buf, sync.v, sync.e)]


KINDS = ("topk-adamw", "signsgd-adamw", "quant-adamw")
LRS = (0.01, 0.02, 0.005, 0.01)


@pytest.mark.parametrize("kind", KINDS)
def test_sync_on_the_device_is_the_cpu_sync_and_a_captured_step_replays_like_it(kind):
    cpu_model, cpu = _sync("cpu", kind)
    dev_model, dev = _sync(DEV, kind)
    grads = _grads(cpu_model, 0)
    for step in range(4):
        cpu.zero_grad(), dev.zero_grad()
        for s in (cpu, dev):
            s.set_hyper(LRS[step], 0.05)
        for p, q, g in zip(cpu_model.parameters(), dev_model.parameters(), grads):
            p.grad, q.grad = g.clone(), g.to(DEV)
        assert cpu.step() == dev.step() == 8 * cpu.bytes_per_step
        assert all(torch.equal(a, b) for a, b in zip(_state(cpu), _state(dev))), step
    assert cpu.e.any() and dev.adam_stats() == cpu.adam_stats() and cpu.adam_stats()["steps"] == 4
    # the same four steps, captured once and replayed (static gradient tensors: the flatten copies them)
    cap_model, cap = _sync(DEV, kind)
    for p, g in zip(cap_model.parameters(), grads):
        p.grad = g.to(DEV)
    cap.set_hyper(LRS[0], 0.05)
    snap, side = cap.snapshot(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cap.step()  # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.step()
    cap.restore(snap)
    for step in range(4):
        cap.set_hyper(LRS[step], 0.05)
        graph.replay()
    assert all(torch.equal(a, b) for a, b in zip(_state(cap), _state(dev)))
    assert cap.adam_stats() == dev.adam_stats()
