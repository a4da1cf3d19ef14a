"""Held-out evaluation without a device: the holdout generators leave the training data bitwise
unchanged, the engine's eval records equal a by-hand evaluation and perturb nothing, two gloo
ranks shard the held-out set exactly once, and the new config keys are validated."""
import os

import pytest
import torch

from network_distributed_pytorch_amd import engine
from network_distributed_pytorch_amd.models import ToyMLP
from network_distributed_pytorch_amd.utils.config import ConfigError, validate_config
from network_distributed_pytorch_amd.utils.data import SyntheticCIFAR10, SyntheticMLPData
from network_distributed_pytorch_amd.utils.launcher import spawn

from . import dist_helpers as H
from .metric_rule import loss_sum_fp64, rule_counts


@pytest.mark.parametrize("seed", [0, 3])
def test_holdout_leaves_training_data_bitwise(seed):
    plain = SyntheticCIFAR10(256, seed=seed)
    train, val = SyntheticCIFAR10(256, seed=seed, holdout=64)
    for k in plain.columns:
        assert torch.equal(train.columns[k], plain.columns[k]), k
    assert len(val) == 64 and val.columns["data"].shape == (64, 3, 32, 32)
    assert val.columns["data"].abs().max() <= 1 and 0 <= int(val.columns["target"].min())
    assert not torch.equal(val.columns["data"], train.columns["data"][:64])
    plain = SyntheticMLPData(200, seed=seed)
    train, val = SyntheticMLPData(200, seed=seed, holdout=50)
    for k in plain.columns:
        assert torch.equal(train.columns[k], plain.columns[k]), k
    assert len(val) == 50 and val.columns["data"].shape == (50, 32)


def _mlp_cfg(**over):
    base = dict(task="mlp", grad_sync="dense", training_epochs=2, dataset_size=128, global_batch=32, verbose=False,
                eval_size=50, eval_topk=2)
    base.update(over)
    return engine.default_config(**base)


def _records(tmp_path, name):
    import json

    with open(os.path.join(tmp_path, name)) as f:
        return [json.loads(line) for line in f]


def test_engine_eval_records_and_no_perturbation(tmp_path):
    torch.manual_seed(0)
    off = engine.run_task(_mlp_cfg(eval_every=0))
    assert "eval" not in off and "eval_s" not in off
    torch.manual_seed(0)
    on = engine.run_task(_mlp_cfg(eval_every=1, log_file=os.path.join(tmp_path, "log.jsonl")))
    assert on["param_checksum"] == off["param_checksum"] and on["epoch_losses"] == off["epoch_losses"]
    recs = on["eval"]
    assert [r["epoch"] for r in recs] == [0, 1]
    assert all(r["n"] == 50 and r["k"] == 2 for r in recs)
    logged = [r for r in _records(tmp_path, "log.jsonl") if r["kind"] == "eval"]
    assert len(logged) == 2
    for key in ("epoch", "loss", "top1", "topk", "n", "k", "eval_s"):
        assert logged[1][key] == recs[1][key]
    # by hand: the final model on the held-out set
    _, val = SyntheticMLPData(128, seed=0, holdout=50)
    model = on["model"]
    assert model.training  # evaluate() restored the mode it found
    model.eval()
    with torch.no_grad():
        logits = model(val.columns["data"].to(next(model.parameters()).device))  # the engine picks the device
    n, c1, ck = rule_counts(logits, val.columns["target"], 2)
    last = recs[1]
    assert (last["n"], last["top1"], last["topk"]) == (n, c1 / n, ck / n)
    ref = loss_sum_fp64(logits, val.columns["target"]) / n
    # 2e-6 (relative + per row) is the fused loss's tolerance against fp64; as much again for the
    # logits themselves, which the engine computes in batches of 32 and this check in one of 50
    assert abs(last["loss"] - ref) <= 4e-6 * abs(ref) + 4e-6
    # evaluating every second epoch of two: one record, after the last epoch
    torch.manual_seed(0)
    two = engine.run_task(_mlp_cfg(eval_every=2))
    assert [r["epoch"] for r in two["eval"]] == [1]
    drop = lambda r: {k: v for k, v in r.items() if k != "eval_s"}  # noqa: E731
    assert drop(two["eval"][0]) == drop(last)


def test_evaluate_topk_none_when_k_covers_all_classes():
    torch.manual_seed(1)
    _, val = SyntheticMLPData(8, seed=1, holdout=20)
    rec = engine.evaluate(ToyMLP(), val, batch=8, topk=4)
    assert rec["topk"] is None and rec["k"] == 4 and rec["n"] == 20 and rec["comm_bytes"] == 0


def eval_rank_body(rank, world, out_dir):
    """Both ranks hold the same weights; each evaluates its shard of 101 held-out rows."""
    from network_distributed_pytorch_amd.parallel.comm import Communicator

    H._init(rank, world)
    torch.manual_seed(5)
    model = ToyMLP()
    _, val = SyntheticMLPData(8, seed=2, holdout=101)
    rec = engine.evaluate(model, val, batch=16, comm=Communicator(), device=torch.device("cpu"), topk=2)
    torch.save(rec, os.path.join(out_dir, f"eval{rank}.pt"))
    torch.distributed.destroy_process_group()


def test_two_ranks_shard_the_heldout_set_once(tmp_path):
    spawn(eval_rank_body, 2, args=(str(tmp_path),))
    recs = [torch.load(os.path.join(tmp_path, f"eval{r}.pt"), weights_only=True) for r in range(2)]
    drop = lambda r: {k: v for k, v in r.items() if k != "eval_s"}  # noqa: E731
    assert drop(recs[0]) == drop(recs[1])
    assert recs[0]["comm_bytes"] == 32  # one fp64[4] all-reduce
    torch.manual_seed(5)
    model = ToyMLP()
    _, val = SyntheticMLPData(8, seed=2, holdout=101)
    single = engine.evaluate(model, val, batch=16, topk=2)
    for key in ("n", "top1", "topk", "k"):
        assert recs[0][key] == single[key], key
    assert recs[0]["n"] == 101
    assert abs(recs[0]["loss"] - single["loss"]) <= 1e-12 * abs(single["loss"])  # fp64 addition order only


@pytest.mark.parametrize("bad", [{"eval_every": -1}, {"eval_topk": 0}, {"eval_size": 0}, {"eval_every": "1"}])
def test_eval_config_validation(bad):
    with pytest.raises(ConfigError):
        validate_config(engine.default_config(**bad))
    out = validate_config({})
    assert (out["eval_every"], out["eval_size"], out["eval_topk"]) == (0, None, 5)
