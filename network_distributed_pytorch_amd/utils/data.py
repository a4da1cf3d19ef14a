"""Synthetic, device-resident datasets with the reference's shapes + an on-device loader.

The reference downloads CIFAR-10 with torchvision (ddp_guide_cifar10/ddp_init.py:37-55)
and tokenizes aclImdb with the HF tokenizer (ddp_powersgd_distillBERT_IMDb/ddp_init.py:
56-94).  Neither torchvision, the datasets nor the network exist on the GPU boxes, so:

* :class:`SyntheticCIFAR10` — 50,000 x (3, 32, 32) float images in [-1, 1] (what
  ``ToTensor + Normalize(0.5, 0.5)`` produces) and 10 labels.  Images carry a
  class-dependent low-frequency pattern under noise so the task is learnable and loss
  curves mean something.
* :class:`SyntheticIMDb` — 25,000 reviews as ``input_ids`` / ``attention_mask`` of length
  512 (the tokenizer's ``truncation=True, padding=True`` output shape), binary labels,
  a label-dependent token distribution, and :func:`train_val_split` with a FIXED seed so
  every rank sees the same split (quirk Q2 fixed: the reference splits per rank with an
  unseeded ``train_test_split``).

Both generate identically on every rank from a seed (so ``DataPartitioner`` shards are
disjoint), and live in HBM: 614 MB for CIFAR is nothing next to 288 GB.
:class:`DeviceLoader` replaces ``DataLoader(partition, batch_size, shuffle=True)``:
per-epoch shuffles and batch gathers happen on the GPU (no host->device copy per step).

Real data: :class:`Uint8ImageDataset` keeps the CIFAR-10 files' images (utils/cifar.py) in HBM as
bytes, 154 MB instead of 614 MB, and assembles every batch with one launch of
``ops.image_batch`` (gather, normalise, random crop + flip, tail padding, targets);
:meth:`DeviceLoader.deliver_into` has the loader write full batches straight into a captured
step's static inputs.
"""
from __future__ import annotations

import math
from typing import Dict, Iterator, Optional, Sequence, Union

import torch

from .partition_helper import Partition

__all__ = ["SyntheticCIFAR10", "SyntheticMLPData", "SyntheticIMDb", "train_val_split", "DeviceLoader",
           "TensorDictDataset", "Uint8ImageDataset", "NORMALIZE"]

# per-channel (mean, std) of config["normalize"]: "half" is the reference's Normalize(0.5, 0.5)
NORMALIZE = {"half": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),
             "cifar": ((0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616))}


class TensorDictDataset:
    """Columns of equal length; ``ds[i]`` returns a dict (or tuple) of row i."""

    def __init__(self, columns: Dict[str, torch.Tensor], as_tuple: Optional[Sequence[str]] = None):
        n = {len(v) for v in columns.values()}
        assert len(n) == 1, "columns must have equal length"
        self.columns = columns
        self.as_tuple = list(as_tuple) if as_tuple else None

    def __len__(self):
        return len(next(iter(self.columns.values())))

    def __getitem__(self, i):
        if self.as_tuple:
            return tuple(self.columns[k][i] for k in self.as_tuple)
        return {k: v[i] for k, v in self.columns.items()}

    def gather(self, idx: torch.Tensor):
        if self.as_tuple:
            return tuple(self.columns[k].index_select(0, idx) for k in self.as_tuple)
        return {k: v.index_select(0, idx) for k, v in self.columns.items()}

    def to(self, device):
        return TensorDictDataset({k: v.to(device) for k, v in self.columns.items()}, self.as_tuple)


class Uint8ImageDataset:
    """Byte images ``[N, C, 32, 32]`` + int64 labels, resident as bytes; batches are assembled by
    :func:`ops.image_batch` (gather, normalise, crop + flip, tail padding: one launch on device).

    Presents the ``columns`` / ``as_tuple`` / ``__len__`` / ``to()`` surface of
    :class:`TensorDictDataset`, so ``DataPartitioner``, :class:`DeviceLoader` and the engine's
    ``Evaluator`` take it as they take any dataset.  ``pad`` / ``flip`` are the augmentation
    ``gather`` applies (and ``gather_into`` with ``augment=True``); which crop and flip a sample
    gets depends on ``(seed, epoch, dataset index)`` only.  ``err`` is the int32 error word an
    out-of-range index sets; :meth:`check_errors` reads it (one host sync).

    ``mix`` (``"mixup"`` / ``"cutmix"`` / ``"mixup_cutmix"``) with ``mix_prob`` turns on
    :func:`ops.image_mix_batch` for the augmented batches: ``gather`` then returns ``(data, target,
    target_b, lam)`` and ``gather_into(augment=True)`` writes the two extra tensors as well.
    ``gather_rows`` and ``gather_into(augment=False)``, hence evaluation, never mix."""

    def __init__(self, images_u8: torch.Tensor, labels: torch.Tensor, mean, std, pad: int = 0, flip: bool = False,
                 mix: str = "none", mix_prob: float = 1.0):
        if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or tuple(images_u8.shape[2:]) != (32, 32):
            raise ValueError(f"Uint8ImageDataset: uint8 [N, C, 32, 32] images expected, got {images_u8.dtype} "
                             f"{tuple(images_u8.shape)}")
        if labels.dim() != 1 or labels.shape[0] != images_u8.shape[0]:
            raise ValueError("Uint8ImageDataset: one label per image expected")
        C = int(images_u8.shape[1])
        self.mean = tuple(float(v) for v in (mean if hasattr(mean, "__len__") else (mean,) * C))
        self.std = tuple(float(v) for v in (std if hasattr(std, "__len__") else (std,) * C))
        if len(self.mean) != C or len(self.std) != C:
            raise ValueError(f"Uint8ImageDataset: mean / std need {C} entries")
        if not 0 <= int(pad) <= 8:
            raise ValueError("Uint8ImageDataset: 0 <= pad <= 8 required")
        self.pad, self.flip = int(pad), bool(flip)
        if mix != "none":
            from ..ops.image_batch import _mix_mode
            _mix_mode(mix, mix_prob)  # ValueError on an unknown mode or a probability outside (0, 1]
        self.mix, self.mix_prob = str(mix), float(mix_prob)
        self.columns = {"data": images_u8.contiguous(), "target": labels.long().contiguous()}
        self.as_tuple = ["data", "target"]
        self.err = torch.zeros(1, dtype=torch.int32, device=images_u8.device)

    def __len__(self):
        return int(self.columns["data"].shape[0])

    def __getitem__(self, i):
        """Row ``i`` unaugmented: (normalised fp32 image, label)."""
        data, target = self.gather_rows(torch.as_tensor([int(i)], device=self.columns["data"].device))
        return data[0], target[0]

    def to(self, device):
        return Uint8ImageDataset(self.columns["data"].to(device), self.columns["target"].to(device), self.mean,
                                 self.std, self.pad, self.flip, self.mix, self.mix_prob)

    def _run_mix(self, idx, out, out_target, out_target_b, out_lam, rows, pad_target, epoch, seed):
        from ..ops.image_batch import image_mix_batch

        return image_mix_batch(self.columns["data"], self.columns["target"], idx, mode=self.mix,
                               mix_prob=self.mix_prob, out=out, out_target=out_target, out_target_b=out_target_b,
                               out_lam=out_lam, rows=rows, mean=self.mean, std=self.std, pad=self.pad, flip=self.flip,
                               seed=seed, epoch=epoch, pad_target=pad_target, err=self.err)

    def _run(self, idx, out, out_target, rows, pad_target, epoch, seed, augment):
        from ..ops.image_batch import image_batch

        return image_batch(self.columns["data"], self.columns["target"], idx, out=out, out_target=out_target,
                           rows=rows, mean=self.mean, std=self.std, pad=self.pad if augment else 0,
                           flip=self.flip and augment, seed=seed, epoch=epoch, pad_target=pad_target, err=self.err)

    def gather_rows(self, idx: torch.Tensor):
        """Fresh unaugmented ``(fp32 batch, targets)``."""
        return self._run(idx, None, None, None, -100, 0, 0, False)

    def gather(self, idx: torch.Tensor, epoch: int = 0, seed: int = 0):
        """Fresh ``(fp32 batch, targets)`` of ``idx``, augmented as the dataset was built; with
        mixing on, ``(fp32 batch, targets, partner targets, lam)``."""
        if self.mix != "none":
            return self._run_mix(idx, None, None, None, None, None, -100, epoch, seed)
        return self._run(idx, None, None, None, -100, epoch, seed, True)

    def gather_into(self, idx: torch.Tensor, data_out: torch.Tensor, target_out: torch.Tensor,
                    target_b_out: Optional[torch.Tensor] = None, lam_out: Optional[torch.Tensor] = None, *,
                    pad_target: int, epoch: int = 0, seed: int = 0, augment: bool = False) -> None:
        """Write the batch of ``idx`` into ``data_out`` / ``target_out`` in place; the rows past
        ``len(idx)`` become zero images with ``target = pad_target``.  With mixing on and
        ``augment=True`` the partner targets and ``lam`` go to ``target_b_out`` / ``lam_out``."""
        if self.mix != "none" and augment:
            if target_b_out is None or lam_out is None:
                raise ValueError("Uint8ImageDataset.gather_into: mixing is on, target_b_out and lam_out are needed")
            self._run_mix(idx, data_out, target_out, target_b_out, lam_out, int(data_out.shape[0]), pad_target,
                          epoch, seed)
            return
        self._run(idx, data_out, target_out, int(data_out.shape[0]), pad_target, epoch, seed, augment)

    def check_errors(self) -> None:
        if int(self.err.item()):
            raise RuntimeError(f"image batch: a sample index was outside [0, {len(self)}) (dataset size "
                               f"{len(self)}); that row was delivered as padding")


def _cifar_images(labels: torch.Tensor, base: torch.Tensor, noise: float, g: torch.Generator) -> torch.Tensor:
    n = len(labels)
    imgs = torch.empty(n, 3, 32, 32)
    chunk = 8192
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        x = base[labels[s:e]] * (1 - noise) + (torch.rand(e - s, 3, 32, 32, generator=g) * 2 - 1) * noise
        imgs[s:e] = x.clamp_(-1, 1)
    return imgs


def SyntheticCIFAR10(n: int = 50000, seed: int = 0, device=None, num_classes: int = 10,
                     noise: float = 0.6, holdout: int = 0):
    """``holdout > 0``: returns ``(train, val)``; the ``holdout`` held-out labels and noise images
    are drawn AFTER the training images from the same generator and class patterns, so ``train``
    is bitwise the dataset of ``holdout=0`` (the patterns depend on how much of the generator
    the labels consumed: never draw ``n + holdout`` labels in one go)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    labels = torch.randint(0, num_classes, (n,), generator=g)
    patterns = torch.rand(num_classes, 3, 4, 4, generator=g) * 2 - 1
    base = torch.nn.functional.interpolate(patterns, size=(32, 32), mode="bilinear", align_corners=False)
    imgs = _cifar_images(labels, base, noise, g)
    ds = TensorDictDataset({"data": imgs, "target": labels}, as_tuple=("data", "target"))
    ds = ds.to(device) if device is not None else ds
    if not holdout:
        return ds
    vlabels = torch.randint(0, num_classes, (int(holdout),), generator=g)
    val = TensorDictDataset({"data": _cifar_images(vlabels, base, noise, g), "target": vlabels},
                            as_tuple=("data", "target"))
    return ds, (val.to(device) if device is not None else val)


def SyntheticMLPData(n: int = 1024, seed: int = 0, device=None, holdout: int = 0):
    """The toy MLP task: 32 Gaussian features, 4 classes = argmax of a fixed random linear map.
    ``holdout > 0``: ``(train, val)``, the held-out features drawn after the training draws from
    the same generator and labelled by the same map (``train`` is bitwise the ``holdout=0`` data)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(n, 32, generator=g)
    w = torch.randn(32, 4, generator=g)
    y = (x @ w).argmax(1)
    ds = TensorDictDataset({"data": x, "target": y}, as_tuple=("data", "target"))
    ds = ds.to(device) if device is not None else ds
    if not holdout:
        return ds
    xv = torch.randn(int(holdout), 32, generator=g)
    val = TensorDictDataset({"data": xv, "target": (xv @ w).argmax(1)}, as_tuple=("data", "target"))
    return ds, (val.to(device) if device is not None else val)


def SyntheticIMDb(n: int = 25000, seq_len: int = 512, vocab: int = 30522, seed: int = 0, device=None,
                  min_len: int = 64) -> TensorDictDataset:
    g = torch.Generator(device="cpu").manual_seed(seed)
    labels = torch.randint(0, 2, (n,), generator=g)
    min_len = max(2, min(min_len, seq_len // 2))
    lengths = torch.randint(min_len, seq_len + 1, (n,), generator=g)
    ids = torch.randint(1000, vocab, (n, seq_len), generator=g)
    # label-dependent "sentiment" tokens sprinkled through each review
    pos_tok = torch.arange(2000, 2050)
    neg_tok = torch.arange(3000, 3050)
    sprinkle = torch.rand(n, seq_len, generator=g) < 0.08
    choice = torch.randint(0, 50, (n, seq_len), generator=g)
    senti = torch.where(labels[:, None].bool(), pos_tok[choice], neg_tok[choice])
    ids = torch.where(sprinkle, senti, ids)
    ids[:, 0] = 101  # [CLS]
    ar = torch.arange(seq_len)[None, :]
    mask = (ar < lengths[:, None]).long()
    ids = torch.where(mask.bool(), ids, torch.zeros_like(ids))  # [PAD] = 0
    ids[torch.arange(n), lengths - 1] = 102  # [SEP]
    ds = TensorDictDataset({"input_ids": ids, "attention_mask": mask, "labels": labels})
    return ds.to(device) if device is not None else ds


def train_val_split(ds: TensorDictDataset, test_size: float = 0.2, seed: int = 42):
    """Fixed-seed split (the reference's ``train_test_split(test_size=.2)``, made rank-identical)."""
    n = len(ds)
    g = torch.Generator(device="cpu").manual_seed(seed)
    perm = torch.randperm(n, generator=g)
    n_test = int(math.ceil(test_size * n))
    test_idx, train_idx = perm[:n_test], perm[n_test:]
    cols_tr = {k: v.index_select(0, train_idx.to(v.device)) for k, v in ds.columns.items()}
    cols_te = {k: v.index_select(0, test_idx.to(v.device)) for k, v in ds.columns.items()}
    return TensorDictDataset(cols_tr, ds.as_tuple), TensorDictDataset(cols_te, ds.as_tuple)


class DeviceLoader:
    """``DataLoader(partition, batch_size, shuffle)`` with on-device shuffling and gathers.

    ``source`` is a :class:`Partition` over a :class:`TensorDictDataset` (or the dataset
    itself).  Each epoch draws a permutation of the shard from a seeded generator.
    """

    def __init__(self, source: Union[Partition, TensorDictDataset], batch_size: int, shuffle: bool = True,
                 seed: int = 0, drop_last: bool = False, device=None):
        if isinstance(source, Partition):
            self.ds = source.data
            self.index = source.index_tensor()
        else:
            self.ds = source
            self.index = torch.arange(len(source))
        first = next(iter(self.ds.columns.values()))
        self.device = torch.device(device) if device is not None else first.device
        if first.device != self.device:
            self.ds = self.ds.to(self.device)
        self.index = self.index.to(self.device)
        self.batch_size = int(batch_size)
        self.shuffle = shuffle
        self.seed = seed
        self.drop_last = drop_last
        self.epoch = 0
        self.dataset = source  # DataLoader-compatible attribute (len(loader.dataset))
        self._static = None

    def deliver_into(self, data: Optional[torch.Tensor], target: Optional[torch.Tensor] = None,
                     pad_target: int = -100, extra: Sequence[torch.Tensor] = ()) -> bool:
        """Have every batch of ``data``'s row count written straight into the caller's
        ``(data, target)`` tensors (e.g. a captured step's static inputs): the loader then yields
        those two tensors themselves instead of fresh ones.  Batches of another size (the ragged
        last one) are still yielded fresh.  Only datasets with ``gather_into`` can do this;
        returns whether delivery is on.  ``deliver_into(None)`` turns it off.  ``extra``: the
        further static tensors of a dataset that mixes samples, ``(target_b, lam)``; they are
        passed on to ``gather_into`` and yielded after ``data`` and ``target``."""
        if data is None or not hasattr(self.ds, "gather_into"):
            self._static = None
            return False
        self._static = (data, target, int(pad_target), tuple(extra))
        return True

    def __len__(self):
        n = len(self.index)
        return n // self.batch_size if self.drop_last else math.ceil(n / self.batch_size)

    def set_epoch(self, epoch: int):
        self.epoch = epoch

    def __iter__(self) -> Iterator:
        n = len(self.index)
        if self.shuffle:
            g = torch.Generator(device="cpu").manual_seed(self.seed * 100003 + self.epoch)
            order = self.index[torch.randperm(n, generator=g).to(self.device)]
        else:
            order = self.index
        epoch = self.epoch
        self.epoch += 1
        keyed = hasattr(self.ds, "gather_into")  # augmentation keyed by (seed, epoch, dataset index)
        for s in range(0, n, self.batch_size):
            e = s + self.batch_size
            if e > n and self.drop_last:
                break
            idx = order[s:e]
            if not keyed:
                yield self.ds.gather(idx)
            elif self._static is not None and len(idx) == self._static[0].shape[0]:
                data, target, pad_target, extra = self._static
                self.ds.gather_into(idx, data, target, *extra, pad_target=pad_target, epoch=epoch, seed=self.seed,
                                    augment=True)
                yield (data, target) + extra
            else:
                yield self.ds.gather(idx, epoch=epoch, seed=self.seed)
