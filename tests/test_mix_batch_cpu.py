"""mixup / CutMix batches on the CPU (ops/image_batch.py: image_mix_batch's torch twin): against the
plain-loop numpy oracle of tests/mix_rule.py bitwise, unmixed rows against ops.image_batch, the error
word, the draw's ranges and distribution, the dataset / loader plumbing, the config keys and a CPU
engine run with the regularisers on."""
import math

import numpy as np
import pytest
import torch

from network_distributed_pytorch_amd import engine, ops
from network_distributed_pytorch_amd.utils.config import ConfigError, validate_config
from network_distributed_pytorch_amd.utils.data import DeviceLoader, Uint8ImageDataset

from .image_rule import MEANSTD, c_hash4, write_fake_cifar
from .mix_rule import oracle_mix_batch, oracle_mix_draw

N = 40
IDX = [(7 * k + 3) % 40 for k in range(13)]  # odd m: the centre row has itself as partner
ROWS = 16  # three padding rows
MODES = ("mixup", "cutmix", "mixup_cutmix")
SEED, EPOCH = 3, 2


def _data(C, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (N, C, 32, 32), dtype=torch.uint8, generator=g),
            torch.randint(0, 10, (N,), generator=g))


_BASE = {}  # (C, flip) -> base images of the oracle, computed once and shared


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mix_prob", [0.5, 1.0])
def test_torch_twin_equals_loop_oracle(C, flip, mode, mix_prob):
    src, labels = _data(C)
    mean, std = (v[:C] for v in MEANSTD["cifar"])
    idx = torch.tensor(IDX, dtype=torch.int64)
    err = torch.zeros(1, dtype=torch.int32)
    kw = dict(rows=ROWS, mean=mean, std=std, pad=4, flip=flip, seed=SEED, epoch=EPOCH, pad_target=-7)
    out, tgt, tgt_b, lam = ops.image_mix_batch(src, labels, idx, mode=mode, mix_prob=mix_prob, err=err, **kw)
    ref, ref_t, ref_tb, ref_lam, ref_err, kinds = oracle_mix_batch(
        src.numpy(), labels.numpy(), IDX, ROWS, mean, std, mode, mix_prob, 4, flip, SEED, EPOCH, -7,
        cache=_BASE.setdefault((C, flip), {}))
    assert out.dtype == torch.float32 and tuple(out.shape) == (ROWS, C, 32, 32)
    assert lam.dtype == torch.float32 and tgt.dtype == tgt_b.dtype == torch.int64
    assert np.array_equal(_bits(out.numpy()), _bits(ref))
    assert np.array_equal(tgt.numpy(), ref_t) and np.array_equal(tgt_b.numpy(), ref_tb)
    assert np.array_equal(_bits(lam.numpy()), _bits(ref_lam))
    assert int(err) == ref_err == 0
    assert kinds[6] == "self" and kinds[13:] == ["pad"] * 3
    n_mixed = sum(k in ("mixup", "cutmix") for k in kinds)
    n_plain = kinds.count("plain")
    print(f"C={C} flip={flip} {mode} p={mix_prob}: {kinds}")
    if mix_prob == 0.5:  # after the self-partner row is excluded
        assert n_mixed >= 3 and n_plain >= 3
        if mode == "mixup_cutmix":
            assert kinds.count("mixup") >= 1 and kinds.count("cutmix") >= 1
            assert (n_mixed, kinds.count("cutmix"), kinds.count("mixup"), n_plain + 1) == (6, 3, 3, 7)
    else:
        assert n_mixed == 12 and n_plain == 0
    # unmixed rows: bitwise ops.image_batch, lam == 1, target_b == target; padding rows likewise
    plain, plain_t = ops.image_batch(src, labels, idx, **kw)
    for b, k in enumerate(kinds):
        if k in ("plain", "self", "pad"):
            assert torch.equal(out[b], plain[b]) and float(lam[b]) == 1.0 and int(tgt_b[b]) == int(tgt[b])
        else:
            assert 0.0 <= float(lam[b]) < 1.0 or k == "cutmix"
            assert int(tgt_b[b]) == int(labels[IDX[12 - b]])
        assert int(tgt[b]) == int(plain_t[b])
    assert float(out[13:].abs().max()) == 0 and bool((tgt[13:] == -7).all()) and bool((tgt_b[13:] == -7).all())


def test_isqrt_by_float_sqrt_is_exact_below_65536():
    """The kernel forms isqrt(u) from sqrtf and corrects it in integers; the uncorrected fp32 value is
    already exact for every u the rule can draw."""
    u = np.arange(65536, dtype=np.int64)
    got = np.floor(np.sqrt(u.astype(np.float32))).astype(np.int64)
    assert np.array_equal(got, np.array([math.isqrt(int(v)) for v in u]))


@pytest.mark.parametrize("mode", MODES)
def test_bad_own_and_bad_partner_index_set_err(mode):
    src, labels = _data(3)
    mean, std = MEANSTD["half"]
    kw = dict(mode=mode, mix_prob=1.0, rows=6, mean=mean, std=std, pad=4, flip=True, seed=SEED, epoch=EPOCH)
    for bad in (N, -1, 2 ** 40):
        idx = [5, bad, 9, 11, 2]  # row 1 has a bad own index, row 3 a bad partner
        err = torch.zeros(1, dtype=torch.int32)
        out, tgt, tgt_b, lam = ops.image_mix_batch(src, labels, torch.tensor(idx), err=err, **kw)
        ref, ref_t, ref_tb, ref_lam, ref_err, kinds = oracle_mix_batch(src.numpy(), labels.numpy(), idx, 6, mean, std,
                                                                       mode, 1.0, 4, True, SEED, EPOCH)
        assert int(err) == ref_err == 1
        assert np.array_equal(_bits(out.numpy()), _bits(ref)) and np.array_equal(_bits(lam.numpy()), _bits(ref_lam))
        assert np.array_equal(tgt.numpy(), ref_t) and np.array_equal(tgt_b.numpy(), ref_tb)
        assert kinds[1] == "pad" and kinds[3] == "plain" and kinds[2] == "self"
        assert float(out[1].abs().max()) == 0 and int(tgt[1]) == int(tgt_b[1]) == -100 and float(lam[1]) == 1.0
        plain, _ = ops.image_batch(src, labels, torch.tensor([11]), mean=mean, std=std, pad=4, flip=True, seed=SEED,
                                   epoch=EPOCH)
        assert torch.equal(out[3], plain[0]) and float(lam[3]) == 1.0 and int(tgt_b[3]) == int(labels[11])
    clean = torch.zeros(1, dtype=torch.int32)
    ops.image_mix_batch(src, labels, torch.tensor([5, 7, 9, 11, 2]), err=clean, **kw)
    assert int(clean) == 0


def test_front_end_rejects_bad_arguments():
    src, labels = _data(3)
    kw = dict(mean=MEANSTD["half"][0], std=MEANSTD["half"][1])
    idx = torch.tensor([0, 1])
    with pytest.raises(ValueError, match="mode"):
        ops.image_mix_batch(src, labels, idx, mode="none", **kw)
    for p in (0.0, -0.5, 1.5, float("nan"), 2.0 ** -30):
        with pytest.raises(ValueError, match="mix_prob"):
            ops.image_mix_batch(src, labels, idx, mode="mixup", mix_prob=p, **kw)
    with pytest.raises(ValueError, match="rows"):
        ops.image_mix_batch(src, labels, idx, mode="mixup", rows=1, **kw)
    with pytest.raises(ValueError, match="out_lam"):
        ops.image_mix_batch(src, labels, idx, mode="mixup", out_lam=torch.empty(1), **kw)
    with pytest.raises(ValueError, match="out_target_b"):
        ops.image_mix_batch(src, labels, idx, mode="mixup", out_target_b=torch.empty(2), **kw)


@pytest.mark.parametrize("seed,epoch", [(3, 2), (714, 0)])
def test_mix_draw_ranges_and_distribution(seed, epoch):
    n = 4096
    draws = [ops.mix_draw(seed, epoch, i, "mixup_cutmix", 0.5) for i in range(n)]
    for i in (0, 1, 77, 4095):  # the Python twin against the C expression of the hash
        d, o = draws[i], oracle_mix_draw(seed, epoch, i, "mixup_cutmix", 0.5)
        assert d[0] == o[0] and (d[1] == "cutmix") == o[1] and np.float32(d[2]) == o[2] and d[3] == o[3]
        assert (c_hash4(seed, epoch, i, 2) >> 8 < (1 << 23)) == d[0]
    mixed = [d for d in draws if d[0]]
    share = len(mixed) / n
    sigma = math.sqrt(0.25 / n)
    print(f"seed {seed} epoch {epoch}: mixed share {share:.4f} (5 sigma = {5 * sigma:.4f})")
    assert abs(share - 0.5) <= 5 * sigma
    assert all(d == (False, None, 1.0, None) for d in draws if not d[0])
    cuts = [d for d in mixed if d[1] == "cutmix"]
    mixups = [d for d in mixed if d[1] == "mixup"]
    assert abs(len(cuts) / len(mixed) - 0.5) <= 5 * math.sqrt(0.25 / len(mixed))
    assert all(d[3] is None and 0.0 <= d[2] < 1.0 and d[2] * (1 << 24) == int(d[2] * (1 << 24)) for d in mixups)
    clipped = unclipped = 0
    for hit, kind, lam, (x0, y0, x1, y1) in cuts:
        assert 0 <= x0 <= x1 <= 32 and 0 <= y0 <= y1 <= 32
        assert lam == 1.0 - (x1 - x0) * (y1 - y0) / 1024.0
        if x1 - x0 == y1 - y0:
            unclipped += 1
        else:
            clipped += 1
    assert clipped > 0 and unclipped > 0
    # mixup's lam is uniform: its mean lies within 5 sigma of one half (sigma^2 = 1 / 12 per draw)
    mean = sum(d[2] for d in mixups) / len(mixups)
    assert abs(mean - 0.5) <= 5 * math.sqrt(1.0 / 12.0 / len(mixups))
    # the other modes draw the same rows, one kind each; mix_prob = 1 draws every row
    assert [ops.mix_draw(seed, epoch, i, "mixup", 0.5)[:2] for i in range(64)] == \
        [(d[0], "mixup" if d[0] else None) for d in draws[:64]]
    assert [ops.mix_draw(seed, epoch, i, "cutmix", 0.5)[:2] for i in range(64)] == \
        [(d[0], "cutmix" if d[0] else None) for d in draws[:64]]
    assert all(ops.mix_draw(seed, epoch, i, "cutmix", 1.0)[0] for i in range(256))


def _u8_dataset(mix, mix_prob=0.5, n=23):
    g = torch.Generator().manual_seed(3)
    return Uint8ImageDataset(torch.randint(0, 256, (n, 3, 32, 32), dtype=torch.uint8, generator=g),
                             torch.randint(0, 10, (n,), generator=g), *MEANSTD["cifar"], pad=4, flip=True, mix=mix,
                             mix_prob=mix_prob)


def test_dataset_and_loader_carry_the_extra_tensors():
    ds = _u8_dataset("mixup_cutmix")
    plain = _u8_dataset("none")
    cols = ds.columns
    loader = DeviceLoader(ds, 5, shuffle=True, seed=4)
    loader.set_epoch(3)
    fresh = [tuple(t.clone() for t in b) for b in loader]
    assert [len(b) for b in fresh] == [4] * 5 and [len(b[0]) for b in fresh] == [5, 5, 5, 5, 3]
    order = torch.randperm(23, generator=torch.Generator().manual_seed(4 * 100003 + 3))
    for k, b in enumerate(fresh):
        ref = ops.image_mix_batch(cols["data"], cols["target"], order[5 * k: 5 * k + 5], mode="mixup_cutmix",
                                  mix_prob=0.5, mean=ds.mean, std=ds.std, pad=4, flip=True, seed=4, epoch=3)
        assert all(torch.equal(x, y) for x, y in zip(b, ref))
    assert any(bool((b[3] != 1).any()) for b in fresh)
    # delivery into caller-owned tensors: the same values, the caller's four tensors for full batches
    static = (torch.empty(5, 3, 32, 32), torch.empty(5, dtype=torch.int64), torch.empty(5, dtype=torch.int64),
              torch.empty(5))
    again = DeviceLoader(ds, 5, shuffle=True, seed=4)
    again.set_epoch(3)
    assert again.deliver_into(static[0], static[1], extra=static[2:])
    for k, b in enumerate(again):
        assert len(b) == 4 and all(x is s for x, s in zip(b, static)) == (k < 4)
        assert all(torch.equal(x, y) for x, y in zip(b, fresh[k]))
    with pytest.raises(ValueError, match="target_b_out"):
        ds.gather_into(order[:5], static[0], static[1], pad_target=-100, augment=True)
    # evaluation's paths never mix: two tensors, bitwise the dataset without mixing
    idx = order[:5]
    for a, b in zip(ds.gather_rows(idx), plain.gather_rows(idx)):
        assert torch.equal(a, b)
    assert len(ds.gather_rows(idx)) == 2 and len(ds[0]) == 2
    d0, t0 = torch.empty(5, 3, 32, 32), torch.empty(5, dtype=torch.int64)
    d1, t1 = torch.empty(5, 3, 32, 32), torch.empty(5, dtype=torch.int64)
    ds.gather_into(idx, d0, t0, pad_target=-100)
    plain.gather_into(idx, d1, t1, pad_target=-100)
    assert torch.equal(d0, d1) and torch.equal(t0, t1)
    moved = ds.to("cpu")
    assert (moved.mix, moved.mix_prob) == ("mixup_cutmix", 0.5)
    with pytest.raises(ValueError, match="mix"):
        _u8_dataset("cutout")
    ds.check_errors()


def test_config_keys():
    c = validate_config({})
    assert (c["label_smoothing"], c["mix"], c["mix_prob"]) == (0.0, "none", 1.0)
    c = validate_config({"data_root": "/data", "mix": "mixup_cutmix", "mix_prob": 0.5, "label_smoothing": 0.1})
    assert (c["label_smoothing"], c["mix"], c["mix_prob"]) == (0.1, "mixup_cutmix", 0.5)
    assert validate_config({"task": "imdb", "label_smoothing": 0.1})["label_smoothing"] == 0.1
    for v in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(ConfigError, match="label_smoothing"):
            validate_config({"label_smoothing": v})
    for v in (0.0, -0.5, 1.5, float("nan"), float("inf"), 2.0 ** -30):
        with pytest.raises(ConfigError, match="mix_prob"):
            validate_config({"data_root": "/data", "mix": "mixup", "mix_prob": v})
    with pytest.raises(ConfigError, match="mix"):
        validate_config({"data_root": "/data", "mix": "cutout"})
    with pytest.raises(ConfigError, match="data_root"):
        validate_config({"mix": "cutmix"})
    with pytest.raises(ConfigError, match="label_smoothing"):
        validate_config({"label_smoothing": "0.1"})
    validate_config(engine.default_config())  # every default_config key is in the schema


def test_cli_flags_reach_the_config():
    import types

    from network_distributed_pytorch_amd.workloads import _cli

    mod = types.SimpleNamespace(config={})
    args = _cli.build_parser(1).parse_args(["-label_smoothing", "0.1", "-mix", "cutmix", "-mix_prob", "0.25"])
    _cli.apply_args(mod, args, 0, 1, None)
    assert (mod.config["label_smoothing"], mod.config["mix"], mod.config["mix_prob"]) == (0.1, "cutmix", 0.25)
    mod = types.SimpleNamespace(config={})
    _cli.apply_args(mod, _cli.build_parser(1).parse_args([]), 0, 1, None)
    assert not {"label_smoothing", "mix", "mix_prob"} & set(mod.config)


def _run(cfg):
    torch.manual_seed(0)  # the engine builds the model from the current RNG
    return engine.run_task(cfg)


def test_engine_run_with_mix_and_smoothing_cpu(tmp_path):
    """ResNet-18 at global batch 8 with a ragged last batch (8 + 8 + 4): the regularisers change the
    run, the run reproduces itself, and the summary names them only when they are on."""
    write_fake_cifar(str(tmp_path), train_sizes=(6, 5, 4, 3, 2), test_size=7, layouts=("bin",))
    base = dict(task="cifar", model="resnet18", num_classes=10, grad_sync="powersgd", training_epochs=2,
                global_batch=8, eval_every=1, eval_topk=5, normalize="cifar", verbose=False,
                data_root=str(tmp_path), augment="crop_flip")
    on = dict(base, mix="mixup_cutmix", label_smoothing=0.1)
    off = _run(engine.default_config(**base))
    a = _run(engine.default_config(**on))
    b = _run(engine.default_config(**on))
    assert a["steps"] == off["steps"] == 6
    assert a["epoch_losses"] == b["epoch_losses"] and a["param_checksum"] == b["param_checksum"]
    assert a["epoch_losses"] != off["epoch_losses"] and a["param_checksum"] != off["param_checksum"]
    assert all(math.isfinite(v) for v in a["epoch_losses"])
    assert (a["label_smoothing"], a["mix"], a["mix_prob"]) == (0.1, "mixup_cutmix", 1.0)
    assert not {"label_smoothing", "mix", "mix_prob"} & set(off)
    assert len(a["eval"]) == 2 and all(r["n"] == 7 and math.isfinite(r["loss"]) for r in a["eval"])
    only_smooth = _run(engine.default_config(**dict(base, label_smoothing=0.1)))
    assert only_smooth["epoch_losses"] != off["epoch_losses"] and only_smooth["epoch_losses"] != a["epoch_losses"]
