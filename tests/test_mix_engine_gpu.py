"""Training with label smoothing and mixup / CutMix from CIFAR-10 files on the device: the mixed
batches and the soft loss inside the captured step against the eager run, a resumed run against the
uninterrupted one, and both against the run with the feature off."""
import math
import os

import pytest
import torch

from network_distributed_pytorch_amd import engine

from .image_rule import write_fake_cifar

pytestmark = pytest.mark.gpu

BATCH, TRAIN_N, EVAL_N = 32, 104, 40  # 3 full batches + a ragged 8; held-out: one full batch + 8 rows
ON = dict(mix="mixup_cutmix", mix_prob=0.5, label_smoothing=0.1)


def _cfg(root, **over):
    return engine.default_config(**dict(dict(
        task="cifar", model="resnet18", num_classes=10, grad_sync="powersgd", training_epochs=2, global_batch=BATCH,
        eval_every=1, eval_topk=5, graph_mode="auto", verbose=False, data_root=root, augment="crop_flip"), **over))


def _run(cfg):
    torch.manual_seed(0)  # the engine builds the model from the current RNG
    return engine.run_task(cfg)


def _records(out):
    return [{k: v for k, v in r.items() if k != "eval_s"} for r in out["eval"]]


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    d = str(tmp_path_factory.mktemp("cifar"))
    write_fake_cifar(d, train_sizes=(30, 24, 20, 20, 10), test_size=EVAL_N, layouts=("py",))
    return d


@pytest.fixture(scope="module")
def captured(root):
    return _run(_cfg(root, **ON))


def test_captured_step_equals_eager(root, captured):
    assert captured["graph_mode"] == "full" and captured["steps"] == 8 and captured["samples"] == 2 * TRAIN_N
    eager = _run(_cfg(root, graph_mode="none", **ON))
    assert eager["graph_mode"] == "none"
    print("captured:", captured["epoch_losses"], captured["param_checksum"], _records(captured))
    print("eager:   ", eager["epoch_losses"], eager["param_checksum"], _records(eager))
    assert captured["epoch_losses"] == eager["epoch_losses"]
    assert captured["param_checksum"] == eager["param_checksum"]
    assert _records(captured) == _records(eager)
    assert (captured["label_smoothing"], captured["mix"], captured["mix_prob"]) == (0.1, "mixup_cutmix", 0.5)


def test_resume_reproduces_the_uninterrupted_run(root, captured, tmp_path):
    ck = str(tmp_path / "ck")
    first = _run(_cfg(root, training_epochs=1, checkpoint_dir=ck, **ON))
    assert first["epoch_losses"] == captured["epoch_losses"][:1]
    resumed = _run(_cfg(root, resume=os.path.join(ck, "last.pt"), **ON))
    assert resumed["param_checksum"] == captured["param_checksum"]
    assert resumed["epoch_losses"] == captured["epoch_losses"][1:]
    assert _records(resumed) == _records(captured)[1:]


def test_feature_changes_training_and_eval_stays_plain(root, captured):
    off = _run(_cfg(root))
    assert off["graph_mode"] == "full" and off["steps"] == captured["steps"]
    assert off["epoch_losses"] != captured["epoch_losses"] and off["param_checksum"] != captured["param_checksum"]
    assert not {"label_smoothing", "mix", "mix_prob"} & set(off)
    for out in (captured, off):
        recs = _records(out)
        assert len(recs) == 2
        for r in recs:
            assert r["n"] == EVAL_N and all(math.isfinite(r[k]) for k in ("loss", "top1", "topk"))
    assert all(math.isfinite(v) for v in captured["epoch_losses"])
