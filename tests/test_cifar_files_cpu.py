"""utils/cifar.load_cifar10: both published CIFAR-10 layouts, record counts taken from the files,
and the errors for missing directories and malformed files."""
import os
import pickle

import numpy as np
import pytest
import torch

from network_distributed_pytorch_amd.utils.cifar import load_cifar10

from .image_rule import write_fake_cifar


@pytest.fixture(scope="module")
def fake(tmp_path_factory):
    roots = {k: str(tmp_path_factory.mktemp("cifar_" + k)) for k in ("py", "bin")}
    arrays = {k: write_fake_cifar(roots[k], layouts=(k,)) for k in roots}
    for a, b in zip(arrays["py"], arrays["bin"]):
        assert np.array_equal(a, b)  # same seed: the two layouts hold the same data set
    return roots, arrays["py"]


@pytest.mark.parametrize("layout", ["py", "bin"])
@pytest.mark.parametrize("direct", [False, True])
def test_layouts_load_identically(fake, layout, direct):
    roots, (tr_x, tr_y, te_x, te_y) = fake
    root = os.path.join(roots[layout], "cifar-10-batches-" + layout) if direct else roots[layout]
    x, y = load_cifar10(root, train=True)
    assert x.dtype == torch.uint8 and tuple(x.shape) == (21, 3, 32, 32) and x.is_contiguous()
    assert y.dtype == torch.int64 and tuple(y.shape) == (21,)
    assert np.array_equal(x.numpy(), tr_x) and np.array_equal(y.numpy(), tr_y)
    x, y = load_cifar10(root, train=False)
    assert x.dtype == torch.uint8 and tuple(x.shape) == (6, 3, 32, 32)
    assert np.array_equal(x.numpy(), te_x) and np.array_equal(y.numpy(), te_y)


def test_missing_directory_names_paths_and_no_download(tmp_path):
    root = str(tmp_path / "nowhere")
    with pytest.raises(FileNotFoundError) as e:
        load_cifar10(root, train=False)
    msg = str(e.value)
    for p in (os.path.join(root, "cifar-10-batches-py", "test_batch"), os.path.join(root, "test_batch"),
              os.path.join(root, "cifar-10-batches-bin", "test_batch.bin"), os.path.join(root, "test_batch.bin")):
        assert p in msg, (p, msg)
    assert "Nothing is downloaded" in msg
    with pytest.raises(FileNotFoundError) as e:
        load_cifar10(root, train=True)
    assert os.path.join(root, "cifar-10-batches-bin", "data_batch_5.bin") in str(e.value)


def test_truncated_bin_raises(tmp_path):
    write_fake_cifar(str(tmp_path), layouts=("bin",))
    path = tmp_path / "cifar-10-batches-bin" / "test_batch.bin"
    raw = path.read_bytes()
    path.write_bytes(raw[:-1])
    with pytest.raises(ValueError, match="3073"):
        load_cifar10(str(tmp_path), train=False)
    load_cifar10(str(tmp_path), train=True)  # the train files are whole


@pytest.mark.parametrize("data", [np.zeros((4, 3071), np.uint8), np.zeros((4, 3072), np.int64),
                                  np.zeros((4 * 3072,), np.uint8)])
def test_wrongly_shaped_pickle_raises(tmp_path, data):
    d = tmp_path / "cifar-10-batches-py"
    d.mkdir()
    with open(d / "test_batch", "wb") as fh:
        pickle.dump({"data": data, "labels": [0, 1, 2, 3]}, fh, protocol=2)
    with pytest.raises(ValueError, match="3072"):
        load_cifar10(str(tmp_path), train=False)
