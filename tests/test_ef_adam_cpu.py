"""``topk-adamw`` / ``signsgd-adamw`` / ``quant-adamw`` without a device: configuration, the lossless
top-k arm against the dense arm's AdamW, the checkpoint round trip and a two-rank gloo run."""
import os

import pytest
import torch

from network_distributed_pytorch_amd.parallel.comm import Communicator
from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync
from network_distributed_pytorch_amd.utils.config import ConfigError, validate_config
from network_distributed_pytorch_amd.utils.launcher import spawn
from network_distributed_pytorch_amd.workloads._cli import build_parser

from . import dist_helpers as H
from .test_signsgd_cpu import _backward, _model

KINDS = ("topk-adamw", "signsgd-adamw", "quant-adamw")


@pytest.mark.parametrize("kind", KINDS)
def test_kinds_validate_build_and_refuse(kind):
    assert validate_config({"grad_sync": kind})["optimizer"] == "adamw"
    assert build_parser(1).parse_args(["-grad_sync", kind]).grad_sync == kind
    sync = build_grad_sync(kind, _model(0), Communicator(), lr=0.01, betas=(0.8, 0.9), eps=1e-6, decay_1d=False)
    assert (sync.optimizer, sync.beta1, sync.beta2, sync.eps, sync.decay_1d) == ("adamw", 0.8, 0.9, 1e-6, False)
    assert sync.adam_stats() == {"b1pow": 1.0, "b2pow": 1.0, "steps": 0} and not sync.v.any()
    with pytest.raises(ConfigError):
        validate_config({"grad_sync": kind, "optimizer": "nadam"})
    with pytest.raises(ConfigError):
        validate_config({"grad_sync": kind, "overlap": True})
    for bad, match in (({"optimizer": "nadam"}, "unknown optimizer"), ({"betas": (1.0, 0.9)}, "beta1"),
                       ({"overlap": True}, "overlap")):
        with pytest.raises(ValueError, match=match):
            build_grad_sync(kind, _model(0), Communicator(), **bad)
    with pytest.raises(ValueError, match="has no AdamW"):  # the plain kind keeps refusing the optimiser
        build_grad_sync(kind[:-6], _model(0), Communicator(), optimizer="adamw")


def test_lossless_topk_adamw_is_the_dense_arm_bitwise():
    models = [_model(0), _model(0)]
    kw = dict(lr=0.01, optimizer="adamw", betas=(0.9, 0.95), decay_1d=False)
    syncs = [build_grad_sync("topk-adamw", models[0], Communicator(), topk_ratio=1.0, **kw),
             build_grad_sync("dense", models[1], Communicator(), **kw)]
    gens = [torch.Generator().manual_seed(5) for _ in syncs]
    for step in range(3):
        for model, sync, gen in zip(models, syncs, gens):
            sync.set_hyper(0.01 / (step + 1), 0.05)
            _backward(model, sync, gen)
            sync.step()
    topk, dense = syncs
    assert not topk.e.any() and topk.adam_stats() == dense.adam_stats() and dense.adam_stats()["steps"] == 3
    for p, q in zip(models[0].parameters(), models[1].parameters()):
        o, d = topk.offsets[id(p)], dense.offsets[id(q)]
        assert torch.equal(p.detach(), q.detach())
        for a, b in ((topk.buf, dense.buf), (topk.v, dense.v)):
            assert torch.equal(a[o: o + p.numel()], b[d: d + p.numel()])


@pytest.mark.parametrize("kind", KINDS)
def test_state_dict_round_trip_resumes_bitwise_and_refuses_the_sgd_arm(kind):
    def run(model, sync, gen):
        for _ in range(2):
            _backward(model, sync, gen)
            sync.step()

    model = _model(0)
    sync = build_grad_sync(kind, model, Communicator(), lr=0.01, decay_1d=False)
    sync.set_hyper(0.01, 0.05)
    gen = torch.Generator().manual_seed(3)
    run(model, sync, gen)
    weights, sd, rng = {k: v.clone() for k, v in model.state_dict().items()}, sync.state_dict(), gen.get_state()
    run(model, sync, gen)
    resumed = _model(1)
    resumed.load_state_dict(weights)
    sync2 = build_grad_sync(kind, resumed, Communicator(), lr=0.5, decay_1d=False)
    sync2.load_state_dict(sd)
    gen2 = torch.Generator()
    gen2.set_state(rng)
    run(resumed, sync2, gen2)
    assert sd["optimizer"] == "adamw" and sd["steps"] == 2 and sd["decay_1d"] is False and sd["betas"] == (0.9, 0.999)
    assert sync.e.any()
    assert all(torch.equal(getattr(sync, k), getattr(sync2, k)) for k in ("x", "e", "buf", "v"))
    assert sync.adam_stats() == sync2.adam_stats() and sync.adam_stats()["steps"] == 4
    plain = build_grad_sync(kind[:-6], _model(1), Communicator())
    with pytest.raises(ValueError, match="cannot be loaded into each other"):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="cannot be loaded into each other"):
        sync2.load_state_dict(plain.state_dict())


def test_two_gloo_ranks_of_signsgd_adamw_stay_bitwise_equal(tmp_path):
    spawn(H.train_rank_body, 2, args=(str(tmp_path), "signsgd-adamw", 4, False))
    ranks = [torch.load(os.path.join(tmp_path, f"signsgd-adamw_rank{r}.pt"), weights_only=True) for r in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(ranks[0]["params"], ranks[1]["params"]))
    assert all(torch.isfinite(p).all() for p in ranks[0]["params"]) and ranks[0]["losses"] != ranks[1]["losses"]
