"""LAMB / LARS (ops/layerwise.py) without a device: the torch twin against the plain reference and its
bounds (tests/layerwise_rule.py), the refusals, and both gradient-sync kinds on a toy model."""
import pytest
import torch

from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync
from network_distributed_pytorch_amd.utils.config import ConfigError, validate_config

from . import layerwise_rule as L

CPU = torch.device("cpu")


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("div", [1.0, 4.0])
@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_twin_within_the_bounds(kind, div, wd):
    L.check_steps(CPU, kind, div, wd)


def _mlp():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(12, 16), torch.nn.ReLU(), torch.nn.Linear(16, 5))


def _step(sync, model, seed):
    g = torch.Generator().manual_seed(seed)
    sync.zero_grad()
    torch.nn.functional.cross_entropy(model(torch.randn(8, 12, generator=g)), torch.randint(0, 5, (8,), generator=g)).backward()
    sync.step()


@pytest.mark.parametrize("kind", ["dense-lamb", "dense-lars"])
def test_kind_steps_a_toy_model(kind):
    model = _mlp()
    before = [p.detach().clone() for p in model.parameters()]
    sync = build_grad_sync(kind, model, lr=1e-2, decay_1d=False)
    sync.set_hyper(1e-2, 0.01)
    for k in range(2):
        _step(sync, model, k)
    trust = sync.trust_ratios()
    assert trust.shape == (4,) and trust[1] == 1 and trust[3] == 1 and trust[0] != 1  # the biases are exempt
    assert all(not torch.equal(a, p) for a, p in zip(before, model.parameters()))
    assert sync.state_dict()["optimizer"] == kind[6:]
    assert (sync.adam_stats() or {}).get("steps") == (2 if kind == "dense-lamb" else None)


def test_refusals():
    model = _mlp()
    with pytest.raises(ValueError, match="unknown grad sync"):
        build_grad_sync("dense-lion", model)
    with pytest.raises(ValueError, match="optimiser choice"):
        build_grad_sync("dense-lamb", model, optimizer="adamw")
    for bad in ({"lars_coef": 0.0}, {"lars_coef": float("nan")}, {"lars_eps": -1.0}, {"lars_eps": float("inf")}):
        with pytest.raises(ValueError, match="lars_"):
            build_grad_sync("dense-lars", model, **bad)
        with pytest.raises(ConfigError, match="lars_"):
            validate_config({"grad_sync": "dense-lars", **bad})
    with pytest.raises(ConfigError, match="optimiser choice"):
        validate_config({"grad_sync": "dense-lars", "optimizer": "adamw"})
    assert validate_config({"grad_sync": "dense-lamb"})["lars_coef"] == 0.001
    syncs = {k: build_grad_sync(k, _mlp(), lr=1e-2) for k in ("dense", "dense-lamb", "dense-lars")}
    for mine, sync in syncs.items():
        for theirs, other in syncs.items():
            if mine != theirs:
                with pytest.raises(ValueError, match="cannot be loaded into each other"):
                    sync.load_state_dict(other.state_dict())
