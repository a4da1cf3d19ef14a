"""grad_sync="signsgd" without a device: configuration, the 2-rank gloo run against a single-process
simulation of both ranks (the twin path), and the checkpoint round trip."""
import os

import pytest
import torch

from network_distributed_pytorch_amd.ops.signsgd import SignCore
from network_distributed_pytorch_amd.parallel.comm import Communicator
from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync
from network_distributed_pytorch_amd.utils.config import ConfigError, validate_config
from network_distributed_pytorch_amd.utils.launcher import spawn

from . import dist_helpers as H


@pytest.mark.parametrize("bad", [{"overlap": True}, {"optimizer": "adamw"}])
def test_config_and_constructor_refusals(bad):
    assert validate_config({"grad_sync": "signsgd"})["grad_sync"] == "signsgd"
    with pytest.raises(ConfigError):
        validate_config({"grad_sync": "signsgd", **bad})
    with pytest.raises(ValueError, match="out of scope" if "overlap" in bad else "has no AdamW"):
        build_grad_sync("signsgd", torch.nn.Linear(4, 2), Communicator(), **bad)


def _model(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3), torch.nn.BatchNorm2d(8), torch.nn.ReLU(),
                               torch.nn.Flatten(), torch.nn.Linear(8 * 6 * 6, 5))


def _backward(model, sync, gen):
    x, y = torch.randn(16, 3, 8, 8, generator=gen), torch.randint(0, 5, (16,), generator=gen)
    sync.zero_grad()
    torch.nn.functional.cross_entropy(model(x), y).backward()


def test_two_gloo_ranks_are_identical_and_equal_the_simulation(tmp_path):
    spawn(H.train_rank_body, 2, args=(str(tmp_path), "signsgd", 4, False))
    ranks = [torch.load(os.path.join(tmp_path, f"signsgd_rank{r}.pt"), weights_only=True)["params"]
             for r in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*ranks))
    # both ranks in this process: the body's models, seeds and batches; rank 0's weights everywhere
    models = [_model(1000 + r) for r in range(2)]
    models[1].load_state_dict(models[0].state_dict())
    syncs = [build_grad_sync("signsgd", m, Communicator(), lr=0.05, momentum=0.9) for m in models]
    gens = [torch.Generator().manual_seed(7 + r) for r in range(2)]
    s0 = syncs[0]
    both = SignCore("cpu", [(s0.offsets[id(p)], p.numel()) for p in s0.params], s0.numel, 2)
    assert s0.bytes_per_step == 4 * 65 * both.nb == s0.collective_payloads()[0] and both.nb == 6
    for _ in range(4):
        for m, s, g in zip(models, syncs, gens):
            _backward(m, s, g)
            s.phase_pack()
        gathered = torch.stack([s.core.out for s in syncs])
        for s in syncs:
            both.update(s.x, s.buf, gathered, s.lr, s.momentum)
    assert all(torch.equal(a, p.detach()) for a, p in zip(ranks[0], models[0].parameters()))


def test_state_dict_round_trip_resumes_bitwise():
    def run(model, sync, steps, gen):
        for _ in steps:
            _backward(model, sync, gen)
            sync.step()

    model = _model(0)
    sync = build_grad_sync("signsgd", model, Communicator(), lr=0.05, momentum=0.9)
    gen = torch.Generator().manual_seed(3)
    run(model, sync, range(2), gen)
    weights, sd, rng = {k: v.clone() for k, v in model.state_dict().items()}, sync.state_dict(), gen.get_state()
    run(model, sync, range(2), gen)
    resumed = _model(1)
    resumed.load_state_dict(weights)
    sync2 = build_grad_sync("signsgd", resumed, Communicator(), lr=0.01, momentum=0.5)
    sync2.load_state_dict(sd)
    gen2 = torch.Generator()
    gen2.set_state(rng)
    run(resumed, sync2, range(2), gen2)
    assert sd["block"] == 2048 and sync.e.any()
    assert torch.equal(sync.x, sync2.x) and torch.equal(sync.e, sync2.e) and torch.equal(sync.buf, sync2.buf)
    with pytest.raises(ValueError, match="block ="):
        sync2.load_state_dict({**sd, "block": 1024})
