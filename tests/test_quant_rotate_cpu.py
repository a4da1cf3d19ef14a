"""quant_rotate="hadamard" without a device: the transform twin against the fp64 Sylvester matrix, the
residual it buys on heavy tails, what it leaves alone, and the checkpoint rules."""
import os

import pytest
import torch
import torch.distributed as dist

from network_distributed_pytorch_amd.models.mlp import ToyMLP
from network_distributed_pytorch_amd.ops.quant import QuantCore, quant_fwht
from network_distributed_pytorch_amd.parallel.comm import Communicator
from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync
from network_distributed_pytorch_amd.utils.config import ConfigError, validate_config
from network_distributed_pytorch_amd.utils.launcher import spawn

from . import dist_helpers as H

G = 2048


def sylvester():
    """``H[t][u] = (-1)^popcount(t & u)`` in fp64."""
    h = torch.ones(1, 1, dtype=torch.float64)
    for _ in range(11):
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


def test_fwht_twin_is_the_sylvester_product_exactly_on_integers():
    """|v| <= 2^12: every partial sum is an integer below 2^24, so each stage is exact in any order."""
    v = torch.randint(-2 ** 12, 2 ** 12 + 1, (3, G), generator=torch.Generator().manual_seed(0)).float()
    v[0, :2] = torch.tensor([2.0 ** 12, -2.0 ** 12])
    assert torch.equal(quant_fwht(v).double(), v.double() @ sylvester())
    assert torch.equal(quant_fwht(quant_fwht(v)) * 2.0 ** -11, v)


def test_rotation_halves_the_4_bit_residual_on_student_t3_blocks():
    """64 blocks of Student-t(3) (a Gaussian over the root of a chi-square(3) / 3), e = 0, one compress:
    the mean over the blocks of ||e'|| / ||m||, both in the domain the block was quantised in."""
    gen = torch.Generator().manual_seed(0)
    g = torch.randn(64 * G, generator=gen) / (torch.randn(3, 64 * G, generator=gen).square().sum(0) / 3).sqrt()
    rel = {}
    for rotate, scale in (("none", 1.0), ("hadamard", G ** 0.5)):  # ||W(d o g)|| = sqrt(2048) ||g||
        e = torch.zeros(64 * G)
        QuantCore("cpu", [(0, 64 * G)], 64 * G, bits=4, rotate=rotate, rotate_seed=1).compress(g, e)
        rel[rotate] = (e.view(64, G).norm(dim=1) / (scale * g.view(64, G).norm(dim=1))).mean().item()
    print(f"plain {rel['none']:.4f}, rotated {rel['hadamard']:.4f}, ratio {rel['hadamard'] / rel['none']:.3f}")
    assert rel["hadamard"] <= 0.5 * rel["none"]


@pytest.mark.parametrize("bits", [2, 4, 8])
@pytest.mark.parametrize("segs,n,same", [([(0, 2047), (2048, 5)], 2064, True), ([(0, 4097)], 4112, False)])
def test_ragged_blocks_and_rotate_none_are_untouched(segs, n, same, bits):
    gen = torch.Generator().manual_seed(bits)
    g, e0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    runs = []
    for kw in ({}, {"rotate": "none", "rotate_seed": 9}, {"rotate": "hadamard", "rotate_seed": 9}):
        runs.append(e0.clone())
        runs.append(QuantCore("cpu", segs, n, bits=bits, **kw).compress(g, runs[-1]).clone())
    assert torch.equal(runs[0], runs[2]) and torch.equal(runs[1], runs[3])
    assert (torch.equal(runs[0], runs[4]) and torch.equal(runs[1], runs[5])) == same
    # the ragged block behind two rotated ones keeps its plain e' and scale word
    assert torch.equal(runs[0][4096:], runs[4][4096:]) and (same or runs[1][-2] == runs[5][-2])


def _sync(**kw):
    torch.manual_seed(0)
    return build_grad_sync("quant", ToyMLP(), Communicator(), lr=0.05, **kw)


def test_unknown_values_and_checkpoints_of_another_rotation_are_refused():
    for bad in ({"quant_rotate": "haar"}, {"quant_rotate_seed": -1}):
        with pytest.raises(ConfigError, match="quant_rotate"):
            validate_config({"grad_sync": "quant", **bad})
    with pytest.raises(ValueError, match="quant_rotate"):
        _sync(quant_rotate="haar")
    sd = _sync(quant_rotate="hadamard", quant_rotate_seed=7).state_dict()
    assert (sd["rotate"], sd["rotate_seed"]) == ("hadamard", 7)
    _sync(quant_rotate="hadamard", quant_rotate_seed=7).load_state_dict(sd)
    old = {k: v for k, v in _sync().state_dict().items() if not k.startswith("rotate")}
    _sync().load_state_dict(old)  # a checkpoint from before the option counts as "none"
    for theirs, kw in ((sd, {}), (sd, {"quant_rotate": "hadamard", "quant_rotate_seed": 8}),
                       (old, {"quant_rotate": "hadamard"})):
        with pytest.raises(ValueError, match="rotation's domain"):
            _sync(**kw).load_state_dict(theirs)


def rank_body(rank, world, out_dir):
    """ToyMLP (fc1.weight is one full block) from a per-rank seed, 3 rotated steps on per-rank batches."""
    H._init(rank, world)
    torch.manual_seed(1000 + rank)
    model = ToyMLP()
    sync = build_grad_sync("quant", model, Communicator(), lr=0.05, quant_rotate="hadamard", quant_rotate_seed=11)
    gen = torch.Generator().manual_seed(7 + rank)
    for _ in range(3):
        sync.zero_grad()
        x, y = torch.randn(16, 32, generator=gen), torch.randint(0, 4, (16,), generator=gen)
        torch.nn.functional.cross_entropy(model(x), y).backward()
        sync.step()
    torch.save({"x": sync.x, "e": sync.e}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


def test_two_gloo_ranks_with_the_rotation_are_replica_identical(tmp_path):
    spawn(rank_body, 2, args=(str(tmp_path),))
    r0, r1 = (torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=True) for r in range(2))
    assert torch.equal(r0["x"], r1["x"]) and r0["e"].any() and not torch.equal(r0["e"], r1["e"])
