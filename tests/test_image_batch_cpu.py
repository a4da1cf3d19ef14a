"""The byte-image batch rule on the CPU (ops/image_batch.py torch twin): against a plain-loop numpy
oracle bitwise, the normalisation error bound, the hash twin, the (seed, epoch, index)-only
dependence, the draw's distribution, the loader and the three config keys."""
import numpy as np
import pytest
import torch

from network_distributed_pytorch_amd import ops
from network_distributed_pytorch_amd.utils.config import ConfigError, validate_config
from network_distributed_pytorch_amd.utils.data import DeviceLoader, TensorDictDataset, Uint8ImageDataset
from network_distributed_pytorch_amd.utils.partition_helper import DataPartitioner

from .image_rule import MEANSTD, c_hash4, oracle_batch, oracle_draw

N = 11


def _data(C, seed=0):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, 256, (N, C, 32, 32), dtype=torch.uint8, generator=g)
    src[0, :, 0, 0], src[1, :, 31, 31] = 0, 255
    return src, torch.randint(0, 10, (N,), generator=g)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("pad,flip", [(0, False), (0, True), (1, False), (1, True), (4, False), (4, True)])
@pytest.mark.parametrize("normalize", ["half", "cifar"])
def test_torch_rule_equals_loop_oracle(C, pad, flip, normalize):
    src, labels = _data(C)
    mean, std = (v[:C] for v in MEANSTD[normalize])
    idx = torch.tensor([0, N - 1, 5, N, 5], dtype=torch.int64)  # a repeat and one index out of range
    err = torch.zeros(1, dtype=torch.int32)
    out, tgt = ops.image_batch(src, labels, idx, rows=7, mean=mean, std=std, pad=pad, flip=flip, seed=714, epoch=2,
                               pad_target=-7, err=err)
    ref, ref_t, ref_err = oracle_batch(src.numpy(), labels.numpy(), idx.numpy(), 7, mean, std, pad, flip, 714, 2, -7)
    assert out.dtype == torch.float32 and tuple(out.shape) == (7, C, 32, 32)
    assert np.array_equal(out.numpy().view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(tgt.numpy(), ref_t)
    assert int(err) == ref_err == 1
    assert float(out[3].abs().max()) == 0 and float(out[5:].abs().max()) == 0
    assert tgt[3] == -7 and (tgt[5:] == -7).all()
    clean = torch.zeros(1, dtype=torch.int32)
    ops.image_batch(src, labels, idx[:3], mean=mean, std=std, pad=pad, flip=flip, err=clean)
    assert int(clean) == 0


@pytest.mark.parametrize("normalize", ["half", "cifar"])
def test_normalisation_error_bound(normalize):
    """Unaugmented output within ((1 + mean_c) / std_c + |out|) * 2^-24 of (v / 255 - mean_c) / std_c
    in fp64: the roundings of scale_c (times v <= 255), of shift_c and of the result."""
    mean, std = MEANSTD[normalize]
    src = torch.arange(256, dtype=torch.uint8).repeat(12).view(1, 3, 32, 32).contiguous()
    out, _ = ops.image_batch(src, torch.zeros(1, dtype=torch.int64), torch.tensor([0]), mean=mean, std=std)
    worst = 0.0
    for c in range(3):
        exact = (src[0, c].double() / 255.0 - mean[c]) / std[c]
        got = out[0, c].double()
        bound = ((1 + mean[c]) / std[c] + got.abs()) * 2.0 ** -24
        worst = max(worst, float(((got - exact).abs() / bound).max()))
        assert bool(((got - exact).abs() <= bound).all()), (c, worst)
    print(f"normalize={normalize}: worst error / bound = {worst:.3f}")


def test_hash_twin_fixed_values():
    # computed once from the C expression (csrc/counter_hash.h) compiled for the host
    assert ops.hash4(0, 0, 0, 0) == 1294405142
    assert ops.hash4(714, 3, 49999, 1) == 934156411
    assert ops.hash4(0xFFFFFFFF, 0x80000000, 123456789, 0xDEADBEEF) == 2606276069
    for args in ((0, 0, 0, 0), (714, 3, 49999, 1), (0xFFFFFFFF, 0x80000000, 123456789, 0xDEADBEEF), (1, 7, 4095, 0)):
        assert ops.hash4(*args) == c_hash4(*args)
    assert ops.crop_flip_draw(714, 3, 49999, 4) == oracle_draw(714, 3, 49999, 4, True)
    assert ops.crop_flip_draw(5, 0, 9, 0, flip=False) == (0, 0, 0)


def test_sample_depends_on_seed_epoch_index_only():
    src, labels = _data(3)
    kw = dict(mean=MEANSTD["half"][0], std=MEANSTD["half"][1], pad=4, flip=True, seed=9)
    a, ta = ops.image_batch(src, labels, torch.tensor([4, 7, 2]), epoch=1, **kw)
    b, tb = ops.image_batch(src, labels, torch.tensor([2, 0, 1, 3, 7, 4, 4]), rows=9, epoch=1, **kw)
    assert torch.equal(a[0], b[5]) and torch.equal(a[0], b[6]) and torch.equal(a[1], b[4]) and torch.equal(a[2], b[0])
    assert ta[0] == tb[5] and ta[1] == tb[4] and ta[2] == tb[0]
    # another epoch (or seed) changes the draw of at least one of the N samples
    every = torch.arange(N)
    e1, _ = ops.image_batch(src, labels, every, epoch=1, **kw)
    e2, _ = ops.image_batch(src, labels, every, epoch=2, **kw)
    assert not torch.equal(e1, e2)
    assert [ops.crop_flip_draw(9, 1, i, 4) for i in range(N)] != [ops.crop_flip_draw(9, 2, i, 4) for i in range(N)]
    s2, _ = ops.image_batch(src, labels, every, epoch=1, **dict(kw, seed=10))
    assert not torch.equal(e1, s2)


@pytest.mark.parametrize("seed", [714, 0, 1])
@pytest.mark.parametrize("epoch", [0, 1, 7])
def test_draw_distribution(seed, epoch):
    draws = [ops.crop_flip_draw(seed, epoch, i, 4) for i in range(4096)]
    dx = np.array([d[0] for d in draws])
    dy = np.array([d[1] for d in draws])
    fl = np.array([d[2] for d in draws])
    assert dx.min() == dy.min() == -4 and dx.max() == dy.max() == 4 and set(fl) == {0, 1}
    cx = [int((dx == v).sum()) for v in range(-4, 5)]
    cy = [int((dy == v).sum()) for v in range(-4, 5)]
    cells = {}
    for d in draws:
        cells[d] = cells.get(d, 0) + 1
    print(f"seed {seed} epoch {epoch}: dx {min(cx)}-{max(cx)} dy {min(cy)}-{max(cy)} flip {fl.mean():.3f} "
          f"cells {len(cells)} min {min(cells.values())}")
    assert all(364 <= v <= 546 for v in cx + cy), (cx, cy)
    assert 0.47 <= fl.mean() <= 0.53
    assert len(cells) == 162


def _u8_dataset(pad=4, flip=True, n=23):
    g = torch.Generator().manual_seed(3)
    return Uint8ImageDataset(torch.randint(0, 256, (n, 3, 32, 32), dtype=torch.uint8, generator=g),
                             torch.randint(0, 10, (n,), generator=g), *MEANSTD["cifar"], pad=pad, flip=flip)


def _expected_order(part, seed, epoch):
    index = part.index_tensor()
    g = torch.Generator(device="cpu").manual_seed(seed * 100003 + epoch)
    return index[torch.randperm(len(index), generator=g)]


def test_loader_yields_the_rule_for_its_permutation():
    ds = _u8_dataset()
    part = DataPartitioner(ds, [0.5, 0.5]).use(1)  # dataset indices, not shard positions, key the draw
    loader = DeviceLoader(part, 4, shuffle=True, seed=21)
    assert len(part) == 11 and len(loader) == 3
    for epoch in range(2):
        order = _expected_order(part, 21, epoch)
        batches = list(loader)
        assert [len(b[0]) for b in batches] == [4, 4, 3]
        for k, (data, target) in enumerate(batches):
            idx = order[4 * k: 4 * k + 4]
            ref, ref_t = ops.image_batch(ds.columns["data"], ds.columns["target"], idx, mean=ds.mean, std=ds.std,
                                         pad=4, flip=True, seed=21, epoch=epoch)
            assert torch.equal(data, ref) and torch.equal(target, ref_t)
            if epoch == 0 and k == 2:  # and against the loop oracle once
                o, t, _ = oracle_batch(ds.columns["data"].numpy(), ds.columns["target"].numpy(), idx.numpy(), 3,
                                       ds.mean, ds.std, 4, True, 21, 0)
                assert np.array_equal(data.numpy(), o) and np.array_equal(target.numpy(), t)
    ds.check_errors()


def test_loader_set_epoch_and_static_delivery():
    ds = _u8_dataset()
    fresh = DeviceLoader(ds, 5, shuffle=True, seed=4)
    epochs = [[(d.clone(), t.clone()) for d, t in fresh] for _ in range(4)]
    again = DeviceLoader(ds, 5, shuffle=True, seed=4)
    again.set_epoch(3)
    fourth = list(again)
    assert len(fourth) == len(epochs[3]) == 5
    for (d, t), (d0, t0) in zip(fourth, epochs[3]):
        assert torch.equal(d, d0) and torch.equal(t, t0)
    assert not torch.equal(epochs[0][0][0], epochs[3][0][0])
    # delivery into caller-owned tensors: the same values, the caller's tensors for full batches
    data, target = torch.empty(5, 3, 32, 32), torch.empty(5, dtype=torch.int64)
    static = DeviceLoader(ds, 5, shuffle=True, seed=4)
    static.set_epoch(3)
    assert static.deliver_into(data, target)
    for k, (d, t) in enumerate(static):
        assert (d is data and t is target) == (k < 4)  # the ragged last batch (3 rows) is fresh
        assert torch.equal(d, epochs[3][k][0]) and torch.equal(t, epochs[3][k][1])


def test_loader_over_tensor_dict_dataset_is_unchanged():
    g = torch.Generator().manual_seed(0)
    cols = {"data": torch.randn(10, 3, generator=g), "target": torch.randint(0, 4, (10,), generator=g)}
    ds = TensorDictDataset(cols, as_tuple=("data", "target"))
    loader = DeviceLoader(ds, 4, shuffle=True, seed=2)
    assert not loader.deliver_into(torch.empty(4, 3), torch.empty(4, dtype=torch.int64))
    for epoch in range(2):
        order = torch.randperm(10, generator=torch.Generator().manual_seed(2 * 100003 + epoch))
        got = list(loader)
        assert [len(b[0]) for b in got] == [4, 4, 2]
        for k, (d, t) in enumerate(got):
            idx = order[4 * k: 4 * k + 4]
            assert torch.equal(d, cols["data"][idx]) and torch.equal(t, cols["target"][idx])
    dl = DeviceLoader(TensorDictDataset(cols), 4, shuffle=False)
    first = next(iter(dl))
    assert set(first) == {"data", "target"} and torch.equal(first["data"], cols["data"][:4])


def test_config_keys():
    c = validate_config({})
    assert (c["data_root"], c["augment"], c["normalize"]) == (None, "none", "half")
    c = validate_config({"data_root": "/data", "augment": "crop_flip", "normalize": "cifar"})
    assert (c["data_root"], c["augment"], c["normalize"]) == ("/data", "crop_flip", "cifar")
    with pytest.raises(ConfigError, match="augment"):
        validate_config({"data_root": "/data", "augment": "mixup"})
    with pytest.raises(ConfigError, match="normalize"):
        validate_config({"normalize": "imagenet"})
    with pytest.raises(ConfigError, match="data_root"):
        validate_config({"data_root": 3})
    with pytest.raises(ConfigError, match="cifar"):
        validate_config({"data_root": "/data", "task": "mlp"})
    with pytest.raises(ConfigError, match="data_root"):
        validate_config({"augment": "crop_flip"})
    from network_distributed_pytorch_amd import engine

    validate_config(engine.default_config())  # every default_config key is in the schema
