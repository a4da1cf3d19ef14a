"""Reader for the published CIFAR-10 files (nothing is ever downloaded).

Two layouts, found either inside ``root`` or with ``root`` being the directory itself:

* ``cifar-10-batches-py``: pickles ``data_batch_1..5`` / ``test_batch`` (``encoding="latin1"``)
  with ``data`` uint8 ``[n, 3072]`` and ``labels``;
* ``cifar-10-batches-bin``: ``data_batch_1..5.bin`` / ``test_batch.bin``, records of one label
  byte followed by 3072 pixel bytes.

The number of records per file is taken from the file.  The reference gets the same arrays from
``torchvision.datasets.CIFAR10(download=True)`` (ddp_powersgd_guide_cifar10/ddp_init.py:40-58).
"""
from __future__ import annotations

import os
import pickle
from typing import List, Tuple

import numpy as np
import torch

__all__ = ["load_cifar10", "CIFAR_PY_DIR", "CIFAR_BIN_DIR"]

CIFAR_PY_DIR = "cifar-10-batches-py"
CIFAR_BIN_DIR = "cifar-10-batches-bin"
_RECORD = 1 + 3072


def _names(train: bool, suffix: str) -> List[str]:
    return [f"data_batch_{i}{suffix}" for i in range(1, 6)] if train else [f"test_batch{suffix}"]


def _read_pickle(path: str) -> Tuple[np.ndarray, np.ndarray]:
    with open(path, "rb") as fh:
        d = pickle.load(fh, encoding="latin1")
    data = d.get("data") if isinstance(d, dict) else None
    if not isinstance(data, np.ndarray) or data.dtype != np.uint8 or data.ndim != 2 or data.shape[1] != 3072:
        got = f"{data.dtype} {data.shape}" if isinstance(data, np.ndarray) else type(data).__name__
        raise ValueError(f"{path}: 'data' must be uint8 [n, 3072], got {got}")
    labels = np.asarray(d.get("labels"), dtype=np.int64).reshape(-1)
    if labels.shape[0] != data.shape[0]:
        raise ValueError(f"{path}: {labels.shape[0]} labels for {data.shape[0]} images")
    return data, labels


def _read_bin(path: str) -> Tuple[np.ndarray, np.ndarray]:
    raw = np.fromfile(path, dtype=np.uint8)
    if raw.size == 0 or raw.size % _RECORD:
        raise ValueError(f"{path}: {raw.size} bytes is not a whole number of {_RECORD}-byte records")
    rec = raw.reshape(-1, _RECORD)
    return rec[:, 1:], rec[:, 0].astype(np.int64)


def load_cifar10(root: str, train: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(uint8 [N, 3, 32, 32], int64 [N])`` of the train (``data_batch_1..5``, in that order) or
    test split found under ``root``."""
    root = os.fspath(root)
    tried = []
    for sub, suffix, read in ((CIFAR_PY_DIR, "", _read_pickle), (CIFAR_BIN_DIR, ".bin", _read_bin)):
        for d in (os.path.join(root, sub), root):
            paths = [os.path.join(d, n) for n in _names(train, suffix)]
            tried.extend(paths)
            if not all(os.path.isfile(p) for p in paths):
                continue
            parts = [read(p) for p in paths]
            images = np.ascontiguousarray(np.concatenate([p[0] for p in parts]).reshape(-1, 3, 32, 32))
            labels = np.concatenate([p[1] for p in parts])
            return torch.from_numpy(images), torch.from_numpy(labels)
    raise FileNotFoundError(
        f"no CIFAR-10 {'train' if train else 'test'} files under {root!r}; tried " + ", ".join(tried)
        + ". Nothing is downloaded: put the extracted "
        f"{CIFAR_PY_DIR} or {CIFAR_BIN_DIR} directory there.")
