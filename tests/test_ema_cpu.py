"""The weight EMA without a GPU: the torch twin and ``ema_decay_at`` against the test-only rule
(tests/ema_rule.py), the condition on the GPU test's inputs (they tell the rule from its fused
variant), swap, the config keys, the engine on the CPU MLP task and two gloo ranks."""
import json
import math
import os
import warnings

import numpy as np
import pytest
import torch

from network_distributed_pytorch_amd import engine, ops
from network_distributed_pytorch_amd.utils.config import ConfigError, validate_config
from network_distributed_pytorch_amd.utils.launcher import spawn

from . import ema_cases as C
from . import ema_dist_helpers as H
from . import ema_rule as R

F = np.float32


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().contiguous().view(torch.int32).numpy().copy()


# ---- twin against the rule -----------------------------------------------------------------------
@pytest.mark.parametrize("decay,updates", [(0.5, 12), (0.999, 12)])
@pytest.mark.parametrize("warmup", [True, False])
def test_twin_and_schedule_equal_rule(decay, updates, warmup):
    shapes = [(5,), (3, 7), (), (2049,)]
    sx, ss = R.special_pairs()
    xs = [torch.from_numpy(R.gaussians(10 + i, int(np.prod(s, dtype=np.int64))).reshape(s)) for i, s in enumerate(shapes)]
    xs.append(torch.from_numpy(sx.copy()))
    ema = ops.WeightEma(xs, decay, warmup=warmup)
    assert ema.read() == {"decay": 0.0, "weight": 0.0, "updates": 0}
    for x, s in zip(xs, ema.shadow):
        assert s.shape == x.shape and np.array_equal(_bits(s), _bits(x))  # the shadow starts as a copy
    ema.shadow[-1].copy_(torch.from_numpy(ss))  # the special pairs: x == s, +-0, +-inf, NaN
    ref = [s.numpy().copy() for s in ema.shadow]
    both = set()
    for n in range(updates):
        for i, x in enumerate(xs[:-1]):  # the optimiser moved the weights
            x.copy_(torch.from_numpy(R.gaussians(100 * n + i, x.numel()).reshape(tuple(x.shape))))
        d, w = R.rule_decay(decay, n, warmup)
        got = ops.ema_decay_at(decay, n, warmup)
        assert isinstance(got[0], np.float32) and isinstance(got[1], np.float32)
        assert got[0].tobytes() == d.tobytes() and got[1].tobytes() == w.tobytes()
        both.add(bool(d < F(decay)))
        ref = [R.rule_update(x.numpy(), s, w) for x, s in zip(xs, ref)]
        ema.update()
        assert ema.read() == {"decay": float(d), "weight": float(w), "updates": n + 1}
        for s, r in zip(ema.shadow, ref):
            assert R.same_bits(s.numpy(), r)
    if warmup and decay == 0.5:
        assert both == {True, False}  # both branches of the min: (n + 1) / (n + 10) reaches 0.5 at n = 8
        assert R.rule_decay(0.5, 7, True)[0] < F(0.5) and R.rule_decay(0.5, 8, True)[0] == F(0.5)
    # documented consequences, on the first update's special pairs
    sx, ss = R.special_pairs()
    w = R.rule_decay(decay, 0, warmup)[1]
    first = R.rule_update(sx, ss, w)
    assert first[1] == 0 and not np.signbit(first[1])     # a shared -0 becomes +0
    assert np.isnan(first[4]) and np.isnan(first[5])       # x = s = inf gives NaN
    assert first[10] == F(2.5) and first[12] == F(1e-3)    # x == s keeps the shadow


def test_first_warm_update_moves_ninety_percent():
    d, w = R.rule_decay(0.999, 0, True)
    assert d == F(1.0) / F(10.0) and w == F(1.0) - d
    assert R.rule_decay(0.999, 0, False) == (F(0.999), F(1.0) - F(0.999))
    big = R.rule_decay(0.999, 2 ** 32 - 1, True)  # (float)n rounds to 2^32; the min picks decay
    assert big[0] == F(0.999)


# ---- the GPU test's inputs tell the rule from fma(w, t, s) ----------------------------------------
def test_gpu_inputs_discriminate_fused_variant():
    tables = [C.main_table()] + [[(n, 0, 0)] for n in C.ONE_ENTRY]
    for cases in tables:
        live, shadow, ls, ss = C.buffers(cases)
        for decay, n, warmup in ((0.999, 0, True), (0.999, 1, True), (0.5, 3, False)):
            w = R.rule_decay(decay, n, warmup)[1]
            differs = 0
            for case, a, b in zip(cases, ls, ss):
                x, s = live[a: a + case[0]], shadow[b: b + case[0]]
                assert np.all(np.isfinite(x)) and np.all(np.abs(x) >= np.finfo(F).tiny)
                assert np.all(np.isfinite(s)) and np.all(np.abs(s) >= np.finfo(F).tiny)
                k = int(np.count_nonzero(R.rule_update(x, s, w).view(np.uint32) != R.fused_update(x, s, w).view(np.uint32)))
                if case[0] >= 1023 and w != F(0.5):  # w = 0.5: the product is exact, both rules agree
                    assert k > 0, (case, decay, n)
                differs += k
            if w != F(0.5):
                assert differs > 0
    # the schedule test's inputs (seeded per step) as well
    x, s = R.gaussians(C.SEED + 5, 4097), R.gaussians(C.SEED + 6, 4097)
    w = R.rule_decay(0.5, 0, True)[1]
    assert np.any(R.rule_update(x, s, w).view(np.uint32) != R.fused_update(x, s, w).view(np.uint32))


# ---- swap, arena, argument checks -----------------------------------------------------------------
def test_swap_is_bitwise_and_an_involution():
    x, s = R.special_pairs()
    nan_payload = np.array([0x7fc12345, 0xffc00001], dtype=np.uint32).view(F)
    xs = [torch.from_numpy(np.concatenate([x, nan_payload])), torch.from_numpy(R.gaussians(1, 33).reshape(3, 11))]
    ema = ops.WeightEma(xs, 0.9)
    ema.shadow[0].copy_(torch.from_numpy(np.concatenate([s, nan_payload[::-1]])))
    ema.shadow[1].copy_(torch.from_numpy(R.gaussians(2, 33).reshape(3, 11)))
    x0, s0 = [_bits(t) for t in xs], [_bits(t) for t in ema.shadow]
    ema.swap()
    assert all(np.array_equal(_bits(a), b) for a, b in zip(xs, s0))
    assert all(np.array_equal(_bits(a), b) for a, b in zip(ema.shadow, x0))
    ema.swap()
    assert all(np.array_equal(_bits(a), b) for a, b in zip(xs, x0))
    assert all(np.array_equal(_bits(a), b) for a, b in zip(ema.shadow, s0))
    assert ema.read()["updates"] == 0


def test_arena_follows_live_alignment_and_state_round_trip():
    base = torch.zeros(64)
    xs = [base[1:6], base[8:12], torch.ones(3, 2)]  # 4 floats past, aligned, own storage
    ema = ops.WeightEma(xs, 0.75, warmup=False)
    for x, s in zip(xs, ema.shadow):
        assert s.data_ptr() % 16 == x.data_ptr() % 16
    for _ in range(3):
        for x in xs:
            x.add_(1.0)
        ema.update()
    sd = ema.state_dict(["a", "b", "c"])
    assert list(sd["shadow"]) == ["a", "b", "c"] and sd["updates"] == 3
    snap = ema.snapshot()
    ema.update()
    ema.restore(snap)
    assert ema.read()["updates"] == 3 and all(torch.equal(sd["shadow"][k], s) for k, s in zip("abc", ema.shadow))
    other = ops.WeightEma([x.clone() for x in xs], 0.75, warmup=False)
    other.load_state_dict(sd)
    assert other.read() == ema.read()
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(other.shadow, ema.shadow))
    with pytest.raises(ValueError):
        ema.state_dict(["a"])
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan"), 1.0 - 1e-12):
        with pytest.raises(ValueError, match="decay"):
            ops.WeightEma(xs, bad)
    with pytest.raises(ValueError, match="float32"):
        ops.WeightEma([torch.zeros(3, dtype=torch.float64)], 0.5)
    with pytest.raises(ValueError, match="contiguous"):
        ops.WeightEma([torch.zeros(4, 4).t()], 0.5)


def test_config_keys():
    c = validate_config({})
    assert c["ema_decay"] == 0.0 and c["ema_warmup"] is True
    d = engine.default_config()
    assert d["ema_decay"] == 0.0 and d["ema_warmup"] is True
    c = validate_config({"ema_decay": 0.999, "ema_warmup": 0})
    assert c["ema_decay"] == 0.999 and c["ema_warmup"] is False
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf"), 1.0 - 1e-12):
        with pytest.raises(ConfigError, match="ema_decay"):
            validate_config({"ema_decay": bad})
    with pytest.raises(ConfigError, match="ema_warmup"):
        validate_config({"ema_warmup": "yes"})
    from network_distributed_pytorch_amd.workloads import _cli

    a = _cli.build_parser(1).parse_args(["-ema_decay", "0.99", "-ema_warmup", "0"])
    assert a.ema_decay == 0.99 and a.ema_warmup == 0
    a = _cli.build_parser(1).parse_args([])
    assert a.ema_decay is None and a.ema_warmup is None


# ---- the engine on the CPU MLP task ---------------------------------------------------------------
STEP_KEYS = ["bytes_per_step", "epoch", "kind", "loss", "payload_bytes", "rank", "samples_per_s", "step", "step_ms",
             "time", "wire_bytes"]
EPOCH_KEYS = ["bytes_per_step", "comm", "epoch", "kind", "mean_loss", "num_batches", "phase_ms", "rank", "steps",
              "time"]
EVAL_KEYS = ["comm_bytes", "epoch", "eval_s", "k", "kind", "loss", "n", "rank", "time", "top1", "topk"]
SUMMARY_KEYS = ["bytes_per_step", "comm", "comm_backend", "elapsed_s", "epoch_losses", "eval", "eval_s", "graph_mode",
                "kind", "param_checksum", "per_rank_batch", "rank", "samples", "samples_per_s", "steps", "time",
                "world_size"]
RETURN_KEYS = sorted(set(SUMMARY_KEYS) - {"kind", "rank", "time"} | {"model", "sync"})


def _run(tmp_path, name, grad_sync="powersgd", epochs=2, **kw):
    cfg = engine.default_config(task="mlp", grad_sync=grad_sync, dataset_size=256, global_batch=32,
                                training_epochs=epochs, verbose=False, learning_rate=0.05, eval_every=1, eval_size=64,
                                log_file=str(tmp_path / f"{name}.jsonl"), **kw)
    torch.manual_seed(1)
    out = engine.run_task(cfg)
    recs = [json.loads(ln) for ln in (tmp_path / f"{name}.jsonl").read_text().splitlines()]
    return out, recs


def test_engine_off_keeps_parent_record_keys(tmp_path):
    for tag, kw in (("default", {}), ("zero", {"ema_decay": 0.0, "ema_warmup": False})):
        out, recs = _run(tmp_path, tag, **kw)
        for kind, keys in (("step", STEP_KEYS), ("epoch", EPOCH_KEYS), ("eval", EVAL_KEYS), ("summary", SUMMARY_KEYS)):
            got = [r for r in recs if r["kind"] == kind]
            assert got and all(sorted(r) == keys for r in got), (kind, sorted(got[0]))
        assert sorted(out) == RETURN_KEYS
        assert out["sync"].opt.ema is None


@pytest.mark.parametrize("grad_sync", ["powersgd", "dense", "powersgd-ref", "powersgd-api", "dense-ref",
                                       "local-sgd-nesterov"])
def test_engine_ema_records_and_no_effect_on_training(tmp_path, grad_sync):
    off, recs_off = _run(tmp_path, "off", grad_sync)
    on, recs = _run(tmp_path, "on", grad_sync, ema_decay=0.9)
    for a, b in zip(off["model"].parameters(), on["model"].parameters()):
        assert np.array_equal(_bits(a), _bits(b))  # the EMA never perturbs training
    assert on["param_checksum"] == off["param_checksum"]
    steps = on["steps"]
    assert steps == 16 and on["ema_updates"] == steps and on["ema_decay"] == 0.9 and on["ema_warmup"] is True
    ema = on["ema"]
    assert isinstance(ema, ops.WeightEma) and ema.read()["updates"] == steps
    d, w = R.rule_decay(0.9, steps - 1, True)
    assert ema.read() == {"decay": float(d), "weight": float(w), "updates": steps}
    assert [r["ema_updates"] for r in recs if r["kind"] == "epoch"] == [8, 16]
    assert all(r["ema_decay"] == 0.9 and r["ema_warmup"] is True for r in recs if r["kind"] in ("epoch", "summary"))
    evs, evs_off = [r for r in recs if r["kind"] == "eval"], [r for r in recs_off if r["kind"] == "eval"]
    assert len(evs) == 2
    for r, o in zip(evs, evs_off):
        assert sorted(r) == sorted(EVAL_KEYS + ["ema_loss", "ema_top1", "ema_topk"])
        assert (r["loss"], r["top1"], r["topk"]) == (o["loss"], o["top1"], o["topk"])  # live fields as without
        assert math.isfinite(r["ema_loss"]) and r["ema_loss"] != r["loss"] and 0.0 <= r["ema_top1"] <= 1.0
    # the last ema_loss is the loss of a fresh model holding the shadow
    from network_distributed_pytorch_amd.models import build_model

    names, tensors = engine.ema_targets(on["model"])
    assert len(names) == len(ema.shadow) and all(t.data_ptr() == x.data_ptr() for t, x in zip(tensors, ema.tensors))
    fresh = build_model("mlp", on["model"].state_dict()[names[-1]].shape[0])
    fresh.load_state_dict(ema.state_dict(names)["shadow"], strict=False)
    cfg = engine.default_config(task="mlp", dataset_size=256, global_batch=32, eval_every=1, eval_size=64)
    validate_config(cfg, strict=False)
    val = engine._build_data(cfg, torch.device("cpu"), 1, 0)[2]
    rec = engine.evaluate(fresh, val, batch=32)
    assert rec["loss"] == evs[-1]["ema_loss"] and rec["top1"] == evs[-1]["ema_top1"]


@pytest.mark.parametrize("grad_sync", ["powersgd", "dense"])
def test_engine_resume_reproduces_shadow_bitwise(tmp_path, grad_sync):
    full, _ = _run(tmp_path, "full", grad_sync, ema_decay=0.9)
    ck = tmp_path / "ck"
    _run(tmp_path, "first", grad_sync, epochs=1, ema_decay=0.9, checkpoint_dir=str(ck))
    state = torch.load(ck / "last.pt", map_location="cpu", weights_only=True)  # plain tensors and containers
    assert state["format"].endswith("ckpt-v2") and state["ema"]["updates"] == 8
    assert list(state["ema"]["shadow"]) == engine.ema_targets(full["model"])[0]
    res, recs = _run(tmp_path, "resumed", grad_sync, ema_decay=0.9, resume=str(ck / "last.pt"))
    for a, b in zip(full["model"].parameters(), res["model"].parameters()):
        assert np.array_equal(_bits(a), _bits(b))
    assert res["ema"].read() == full["ema"].read() and res["ema_updates"] == 16
    for a, b in zip(full["ema"].shadow, res["ema"].shadow):
        assert np.array_equal(_bits(a), _bits(b))
    assert [r for r in recs if r["kind"] == "eval"][-1]["ema_loss"] == full["eval"][-1]["ema_loss"]
    # a checkpoint without an EMA, resumed with one: a warning, the shadow starts from the loaded weights
    ck2 = tmp_path / "ck2"
    _run(tmp_path, "plain", grad_sync, epochs=1, checkpoint_dir=str(ck2))
    assert "ema" not in torch.load(ck2 / "last.pt", map_location="cpu", weights_only=True)
    with pytest.warns(UserWarning, match="no weight EMA"):
        late, _ = _run(tmp_path, "late", grad_sync, ema_decay=0.9, resume=str(ck2 / "last.pt"))
    assert late["ema_updates"] == 8
    for a, b in zip(full["model"].parameters(), late["model"].parameters()):
        assert np.array_equal(_bits(a), _bits(b))


def test_checkpoint_shadow_loads_into_a_model(tmp_path):
    from network_distributed_pytorch_amd.utils.checkpoint import load_checkpoint, save_checkpoint

    torch.manual_seed(3)
    model = torch.nn.Sequential(torch.nn.Linear(4, 6), torch.nn.BatchNorm1d(6), torch.nn.Linear(6, 2))
    names, tensors = engine.ema_targets(model)
    assert names == ["0.weight", "0.bias", "1.weight", "1.bias", "2.weight", "2.bias", "1.running_mean", "1.running_var"]
    ema = ops.WeightEma(tensors, 0.5, warmup=False)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(1.0)
    model(torch.randn(8, 4))  # moves the running statistics
    ema.update()
    path = str(tmp_path / "c.pt")
    save_checkpoint(path, model, None, epoch=0, step=1, rank=0, world=1, ema=ema.state_dict(names))
    state = torch.load(path, map_location="cpu", weights_only=True)
    fresh = torch.nn.Sequential(torch.nn.Linear(4, 6), torch.nn.BatchNorm1d(6), torch.nn.Linear(6, 2))
    missing = fresh.load_state_dict(state["ema"]["shadow"], strict=False)
    assert set(missing.missing_keys) <= {"1.num_batches_tracked"} and not missing.unexpected_keys
    for k, s in zip(names, ema.shadow):
        assert torch.equal(fresh.state_dict()[k], s)
    other = ops.WeightEma(engine.ema_targets(fresh)[1], 0.5, warmup=False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        info = load_checkpoint(path, fresh, None, rank=0, world=1, ema=other)
    assert info["ema"]["updates"] == 1 and other.read() == ema.read()
    assert all(torch.equal(a, b) for a, b in zip(other.shadow, ema.shadow))


# ---- two gloo ranks -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "powersgd"])
def test_two_ranks_keep_equal_shadows(tmp_path, kind):
    spawn(H.ema_rank_body, 2, args=(str(tmp_path), kind, 0.9, 4))
    a, b = (torch.load(os.path.join(tmp_path, f"{kind}_rank{r}.pt"), weights_only=True) for r in range(2))
    assert a["block"] == b["block"] and a["block"]["updates"] == 4
    for p, q in zip(a["params"], b["params"]):
        assert torch.equal(p, q)
    for s, t, p in zip(a["shadow"], b["shadow"], a["params"]):
        assert np.array_equal(_bits(s), _bits(t))
        assert not torch.equal(s, p)  # the shadow lags the weights
