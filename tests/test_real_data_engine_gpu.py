"""Training and evaluating from CIFAR-10 files (``data_root``): the byte-image path (one launch per
batch, written into the captured step's static inputs) against the same run fed by fp32 datasets
precomputed from the same bytes by the CPU rule, which takes the gather + copy path."""
import os

import pytest
import torch

from network_distributed_pytorch_amd import engine, ops
from network_distributed_pytorch_amd.utils.data import NORMALIZE, TensorDictDataset
from network_distributed_pytorch_amd.utils.partition_helper import DataPartitioner

from .image_rule import write_fake_cifar


def _precomputed_build_data(arrays, normalize="half"):
    """An ``engine._build_data`` that serves fp32 TensorDictDatasets made by the CPU rule."""
    mean, std = NORMALIZE[normalize]

    def fp32(images, labels, n):
        x, y = torch.from_numpy(images[:n]), torch.from_numpy(labels[:n])
        data, target = ops.image_batch(x, y, torch.arange(len(x)), mean=mean, std=std)
        return TensorDictDataset({"data": data, "target": target}, as_tuple=("data", "target"))

    def build(config, device, world, rank):
        tr_x, tr_y, te_x, te_y = arrays
        ds = fp32(tr_x, tr_y, config["dataset_size"] or len(tr_x)).to(device)
        val = fp32(te_x, te_y, config["eval_size"] or len(te_x)).to(device) if config["eval_every"] else None
        part = DataPartitioner(ds, [1.0 / world for _ in range(world)]).use(rank)
        return part, int(config["global_batch"] / float(world)), val
    return build


def _run(cfg):
    torch.manual_seed(0)  # the engine builds the model from the current RNG
    return engine.run_task(cfg)


def _records(out):
    return [{k: v for k, v in r.items() if k != "eval_s"} for r in out["eval"]]


def _assert_same_run(a, b, n_eval):
    assert a["epoch_losses"] == b["epoch_losses"] and a["steps"] == b["steps"]
    assert a["param_checksum"] == b["param_checksum"]
    assert len(a["eval"]) == len(b["eval"]) == 2
    for ra, rb in zip(_records(a), _records(b)):
        assert ra == rb and ra["n"] == n_eval
        assert set(ra) >= {"loss", "top1", "topk", "n"}


# ---- no GPU needed (runs on whatever device the engine picks): real vs precomputed, ResNet-18 at
# batch 8, with the ragged last training batch and a padded evaluation tail ----------------------

def test_real_data_equals_precomputed_cpu(tmp_path, monkeypatch):
    arrays = write_fake_cifar(str(tmp_path), train_sizes=(6, 5, 4, 3, 2), test_size=7, layouts=("bin",))
    base = dict(task="cifar", model="resnet18", num_classes=10, grad_sync="powersgd", training_epochs=2,
                global_batch=8, eval_every=1, eval_topk=5, normalize="cifar", verbose=False)
    real = _run(engine.default_config(data_root=str(tmp_path), **base))
    assert real["steps"] == 6  # 8 + 8 + 4 per epoch
    monkeypatch.setattr(engine, "_build_data", _precomputed_build_data(arrays, "cifar"))
    pre = _run(engine.default_config(**base))
    _assert_same_run(real, pre, 7)
    monkeypatch.undo()
    capped = _run(engine.default_config(data_root=str(tmp_path), dataset_size=16, eval_size=5,
                                        **dict(base, training_epochs=1)))
    assert capped["steps"] == 2 and capped["eval"][0]["n"] == 5


# ---- GPU: ResNet-18, captured step ---------------------------------------------------------------

BATCH, TRAIN_N, EVAL_N = 32, 96, 40  # held-out: one full batch + 8 rows padded to 32


def _gpu_cfg(root, **over):
    return engine.default_config(**dict(dict(
        task="cifar", model="resnet18", num_classes=10, grad_sync="powersgd", training_epochs=2, global_batch=BATCH,
        eval_every=1, eval_topk=5, graph_mode="auto", verbose=False, data_root=root), **over))


@pytest.fixture(scope="module")
def fake(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    root = str(tmp_path_factory.mktemp("cifar"))
    arrays = write_fake_cifar(root, train_sizes=(30, 20, 20, 16, 10), test_size=EVAL_N, layouts=("py",))
    return root, arrays


@pytest.fixture(scope="module")
def real(fake):
    return _run(_gpu_cfg(fake[0]))


@pytest.fixture(scope="module")
def cropped(fake):
    return _run(_gpu_cfg(fake[0], augment="crop_flip"))


@pytest.mark.gpu
def test_real_data_equals_precomputed(fake, real, monkeypatch):
    assert real["graph_mode"] == "full" and real["steps"] == 6 and real["samples"] == 2 * TRAIN_N
    monkeypatch.setattr(engine, "_build_data", _precomputed_build_data(fake[1]))
    pre = _run(_gpu_cfg(None))
    assert pre["graph_mode"] == "full"
    print("eval records, bytes:", _records(real), "precomputed:", _records(pre))
    _assert_same_run(real, pre, EVAL_N)


@pytest.mark.gpu
def test_crop_flip_changes_training_and_reproduces(fake, real, cropped):
    assert cropped["param_checksum"] != real["param_checksum"]
    assert cropped["epoch_losses"] != real["epoch_losses"]
    again = _run(_gpu_cfg(fake[0], augment="crop_flip"))
    assert again["param_checksum"] == cropped["param_checksum"]
    assert again["epoch_losses"] == cropped["epoch_losses"] and _records(again) == _records(cropped)


@pytest.mark.gpu
def test_resume_reproduces_the_uninterrupted_run(fake, cropped, tmp_path):
    ck = str(tmp_path / "ck")
    first = _run(_gpu_cfg(fake[0], augment="crop_flip", training_epochs=1, checkpoint_dir=ck))
    assert first["epoch_losses"] == cropped["epoch_losses"][:1]
    resumed = _run(_gpu_cfg(fake[0], augment="crop_flip", resume=os.path.join(ck, "last.pt")))
    assert resumed["param_checksum"] == cropped["param_checksum"]
    assert resumed["epoch_losses"] == cropped["epoch_losses"][1:]
    assert _records(resumed) == _records(cropped)[1:]
