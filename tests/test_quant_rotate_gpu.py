"""The rotated instances of csrc/quant.hip on the device: the pack against an fp64 product with the Sylvester
matrix followed by the plain reference of tests/test_quant_gpu.py, against the twin bitwise and within the
11-stage rounding bound; the two updates and the sync against the twin."""
import pytest
import torch

from network_distributed_pytorch_amd.models.mlp import ToyMLP
from network_distributed_pytorch_amd.ops.adamw import AdamState
from network_distributed_pytorch_amd.ops.quant import QuantCore, quant_rotate_signs
from network_distributed_pytorch_amd.parallel.comm import Communicator
from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync

from .test_quant_gpu import _place, _reference
from .test_quant_rotate_cpu import sylvester
from .test_signsgd_gpu import SENTINEL, _bits, _grads, _layout, _state

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
G, SEED = 2048, 0x9E3779B9
ROT = {"rotate": "hadamard", "rotate_seed": SEED}
# a lone full block; a ragged block behind full ones; a full block whose index is not its position
TABLES = ([2048], [4097], [2047, 2048, 5])
table_bits = pytest.mark.parametrize("counts,bits", [(c, b) for c in TABLES for b in (2, 4, 8)],
                                     ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v))


def _rotated64(g, blocks):
    """``H (d o g)`` of every full block in fp64 (a ragged block keeps g) and ``sum |g|`` per element of it."""
    y, mag, H = g.double().clone(), torch.zeros(g.numel(), dtype=torch.float64), sylvester()
    for j, (off, ln) in enumerate(blocks):
        if ln == G:
            y[off: off + G] = (quant_rotate_signs(SEED, j).double() * g[off: off + G].double()) @ H
            mag[off: off + G] = g[off: off + G].double().abs().sum()
    return y, mag


@table_bits
@pytest.mark.parametrize("arm", ["integers", "gaussians"])
def test_pack_is_the_fp64_rotation_then_the_plain_reference_and_the_twin(arm, counts, bits):
    """Row and e' are the twin's bit for bit in both arms.
    integers: |g|, |e| <= 8, so every butterfly sum is an integer below 2^15, exact in any stage order:
    m = H (d o g) + e exactly, and row and e' are the plain rule's on that m.
    gaussians: with e = 0, m is y = W(d o g) itself, and m = c + e' exactly (c = fmul(q, s) lies within s / 2
    of m, so the subtraction that formed e' was exact).  Every output of W is a sum of 2048 terms +-g_t through
    11 roundings: |y - y64| <= gamma_11 sum |g_t|, gamma_11 = 11 u / (1 - 11 u), u = 2^-24."""
    segs, blocks, n, live = _layout(counts)
    nb, cw, L = len(blocks), 64 * bits * len(blocks), 2 ** (bits - 1) - 1
    gen = torch.Generator().manual_seed(n + bits)
    g, e0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    if arm == "integers":
        g, e0 = (torch.randint(-8, 9, (n,), generator=gen).float() for _ in range(2))
    e0[~live] = SENTINEL
    dev, twin = QuantCore(DEV, segs, n, bits=bits, **ROT), QuantCore("cpu", segs, n, bits=bits, **ROT)
    et, ed = e0.clone(), e0.clone().to(DEV)
    out = dev.compress(g.to(DEV), ed).cpu()
    assert torch.equal(out, twin.compress(g, et)) and torch.equal(_bits(ed), _bits(et))
    y64, mag = _rotated64(g, blocks)
    if arm == "integers":
        m = y64 + e0.double()
        words, scales, res, _ = _reference(m.float(), torch.zeros(n), blocks, bits)
        assert torch.equal(m.float().double(), m) and torch.equal(out[:cw].long() & 0xFFFFFFFF, words)
        assert torch.equal(out[cw: cw + nb], scales) and not out[cw + nb:].any()
        assert torch.equal(ed.cpu()[live], res[live]) and torch.equal(_bits(ed)[~live], _bits(e0)[~live])
        return
    ed = torch.zeros(n, device=DEV)
    out = dev.compress(g.to(DEV), ed).cpu()
    gamma = 11 * 2.0 ** -24 / (1 - 11 * 2.0 ** -24)
    for j, (off, ln) in enumerate(blocks):
        if ln == G:
            w, sh = _place(bits, j, torch.arange(G))
            c = (((out[w] >> sh.to(torch.int32)) & (2 ** bits - 1)) - L).float() * out[cw + j].view(torch.float32)
            y = c.double() + ed.cpu()[off: off + G].double()
            err = (y - y64[off: off + G]).abs() / (gamma * mag[off: off + G])
            print(f"block {j}: worst |y - y64| / (gamma_11 sum |g|) = {err.max().item():.4f}")
            assert (err <= 1).all()


@table_bits
@pytest.mark.parametrize("N,wd", [(1, 0.0), (3, 0.0), (1, 5e-4), (3, 5e-4)])
def test_updates_are_the_twin_bitwise(N, wd, counts, bits):
    """SGD and AdamW behind the inverse rotation; padding, gaps and ragged blocks included."""
    segs, blocks, n, live = _layout(counts)
    nb, lr, lam = len(blocks), 0.05, 0.9
    gen = torch.Generator().manual_seed(N + bits)
    x, b, v = torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.rand(n, generator=gen)
    x[~live], b[~live], v[~live] = SENTINEL, -SENTINEL, SENTINEL
    dev, twin = QuantCore(DEV, segs, n, N, bits, **ROT), QuantCore("cpu", segs, n, N, bits, **ROT)
    gathered = torch.randint(-2 ** 31, 2 ** 31, (N, dev.words), generator=gen).to(torch.int32)  # any codes
    gathered[:, 64 * bits * nb: 64 * bits * nb + nb] = (torch.rand(N, nb, generator=gen) + 0.01).view(torch.int32)
    hyper = torch.tensor([lr, wd, 0.0, 0.0], device=DEV)
    xt, bt, xd, bd = x.clone(), b.clone(), x.clone().to(DEV), b.clone().to(DEV)
    twin.update(xt, bt, gathered, lr, lam, wd)
    dev.update(xd, bd, gathered.to(DEV), 0.0, lam, 0.0, hyper)
    assert torch.equal(_bits(xd), _bits(xt)) and torch.equal(_bits(bd), _bits(bt))
    assert not torch.equal(xt[live], x[live]) and torch.equal(_bits(xt)[~live], _bits(x)[~live])
    xt, mt, vt = x.clone(), b.clone(), v.clone()
    xd, md, vd = (t.clone().to(DEV) for t in (x, b, v))
    flags = [i % 2 == 0 for i in range(len(segs))]
    twin.update_adam(xt, mt, vt, gathered, lr, wd, 0.9, 0.95, 1e-8, AdamState("cpu", nb), twin.block_decays(flags))
    dev.update_adam(xd, md, vd, gathered.to(DEV), lr, wd, 0.9, 0.95, 1e-8, AdamState(DEV, nb),
                    dev.block_decays(flags), hyper)
    assert all(torch.equal(_bits(a), _bits(t)) for a, t in ((xd, xt), (md, mt), (vd, vt)))
    assert torch.equal(_bits(vt)[~live], _bits(v)[~live]) and not torch.equal(vt[live], v[live])


def _sync(device, kind, bits):
    torch.manual_seed(0)
    model = ToyMLP().to(device)  # fc1.weight is one full block, every other tensor a ragged one
    return model, build_grad_sync(kind, model, Communicator(), lr=0.05, momentum=0.9, quant_bits=bits,
                                  quant_rotate="hadamard", quant_rotate_seed=SEED)


@pytest.mark.parametrize("bits", [2, 4, 8])
@pytest.mark.parametrize("kind", ["quant", "quant-adamw"])
def test_sync_on_the_device_is_the_cpu_twin_and_a_captured_step_replays_like_it(kind, bits):
    (cpu_model, cpu), (dev_model, dev), (cap_model, cap) = (_sync(d, kind, bits) for d in ("cpu", DEV, DEV))
    grads = _grads(cpu_model, 0)
    for p, g in zip(cap_model.parameters(), grads):
        p.grad = g.to(DEV)  # static gradient tensors: the flatten launch copies them into the arena
    snap, side = cap.snapshot(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cap.step()  # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.step()
    cap.restore(snap)
    for step in range(3):
        cpu.zero_grad(), dev.zero_grad()
        for p, q, g in zip(cpu_model.parameters(), dev_model.parameters(), grads):
            p.grad, q.grad = g.clone(), g.to(DEV)
        assert cpu.step() == dev.step() == 8 * cpu.bytes_per_step
        graph.replay()
        for a, b, c in zip(_state(cpu), _state(dev), _state(cap)):
            assert torch.equal(a, b) and torch.equal(c, b), step
    plain = build_grad_sync(kind, ToyMLP(), Communicator(), quant_bits=bits)
    assert cpu.e.any() and cpu.bytes_per_step == plain.bytes_per_step
