"""grad_sync="quant" without a device: configuration, the 2-rank gloo run against a single-process
simulation of both ranks (the twin path), and the checkpoint round trip."""
import os

import pytest
import torch

from network_distributed_pytorch_amd.ops.quant import QuantCore
from network_distributed_pytorch_amd.parallel.comm import Communicator
from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync
from network_distributed_pytorch_amd.utils.config import ConfigError, validate_config
from network_distributed_pytorch_amd.utils.launcher import spawn
from network_distributed_pytorch_amd.workloads._cli import build_parser

from . import dist_helpers as H
from .test_signsgd_cpu import _backward, _model


@pytest.mark.parametrize("bad,match", [({"quant_bits": 3}, "quant_bits"), ({"overlap": True}, "out of scope"),
                                       ({"optimizer": "adamw"}, "has no AdamW")])
def test_config_constructor_and_flag_refusals(bad, match):
    assert validate_config({"grad_sync": "quant"})["quant_bits"] == 4
    assert validate_config({"grad_sync": "quant", "quant_bits": 2})["quant_bits"] == 2
    with pytest.raises(ConfigError):
        validate_config({"grad_sync": "quant", **bad})
    with pytest.raises(ValueError, match=match):
        build_grad_sync("quant", torch.nn.Linear(4, 2), Communicator(), **bad)
    assert build_parser(1).parse_args(["-grad_sync", "quant", "-quant_bits", "8"]).quant_bits == 8
    with pytest.raises(SystemExit):
        build_parser(1).parse_args(["-quant_bits", "3"])


def test_two_gloo_ranks_are_identical_and_equal_the_simulation(tmp_path):
    spawn(H.train_rank_body, 2, args=(str(tmp_path), "quant", 4, False))
    ranks = [torch.load(os.path.join(tmp_path, f"quant_rank{r}.pt"), weights_only=True)["params"] for r in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*ranks))
    # both ranks in this process: the body's models, seeds and batches; rank 0's weights everywhere
    models = [_model(1000 + r) for r in range(2)]
    models[1].load_state_dict(models[0].state_dict())
    syncs = [build_grad_sync("quant", m, Communicator(), lr=0.05, momentum=0.9) for m in models]
    gens = [torch.Generator().manual_seed(7 + r) for r in range(2)]
    s0 = syncs[0]
    both = QuantCore("cpu", [(s0.offsets[id(p)], p.numel()) for p in s0.params], s0.numel, 2, bits=4)
    assert both.nb == 6 and s0.bytes_per_step == 4 * both.words == 4 * 1544 == s0.collective_payloads()[0]
    for _ in range(4):
        for m, s, g in zip(models, syncs, gens):
            _backward(m, s, g)
            s.phase_pack()
        gathered = torch.stack([s.core.out for s in syncs])
        for s in syncs:
            both.update(s.x, s.buf, gathered, s.lr, s.momentum)
    assert all(torch.equal(a, p.detach()) for a, p in zip(ranks[0], models[0].parameters()))


@pytest.mark.parametrize("bits", [2, 8])
def test_state_dict_round_trip_resumes_bitwise(bits):
    def run(model, sync, gen):
        for _ in range(2):
            _backward(model, sync, gen)
            sync.step()

    model = _model(0)
    sync = build_grad_sync("quant", model, Communicator(), lr=0.05, momentum=0.9, quant_bits=bits)
    gen = torch.Generator().manual_seed(3)
    run(model, sync, gen)
    weights, sd, rng = {k: v.clone() for k, v in model.state_dict().items()}, sync.state_dict(), gen.get_state()
    run(model, sync, gen)
    resumed = _model(1)
    resumed.load_state_dict(weights)
    sync2 = build_grad_sync("quant", resumed, Communicator(), lr=0.01, momentum=0.5, quant_bits=bits)
    sync2.load_state_dict(sd)
    gen2 = torch.Generator()
    gen2.set_state(rng)
    run(resumed, sync2, gen2)
    assert (sd["block"], sd["bits"]) == (2048, bits) and sync.e.any()
    assert torch.equal(sync.x, sync2.x) and torch.equal(sync.e, sync2.e) and torch.equal(sync.buf, sync2.buf)
    with pytest.raises(ValueError, match="bits ="):
        build_grad_sync("quant", _model(1), Communicator(), quant_bits=4).load_state_dict(sd)
