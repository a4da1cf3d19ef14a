"""Test-side helpers for the byte-image path: fake CIFAR-10 files in both published layouts and a
plain-loop numpy oracle of the batch rule (ops/image_batch.py), written independently of it."""
import os
import pickle

import numpy as np

MEANSTD = {"half": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),
           "cifar": ((0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616))}

M32 = 0xFFFFFFFF


def write_fake_cifar(root, train_sizes=(7, 5, 4, 3, 2), test_size=6, seed=0, layouts=("py", "bin")):
    """Random bytes in the CIFAR-10 layouts under ``root``; returns the arrays written:
    ``(train_images [N,3,32,32] u8, train_labels [N] i64, test_images, test_labels)``."""
    rng = np.random.default_rng(seed)
    files = [(f"data_batch_{k + 1}", n) for k, n in enumerate(train_sizes)] + [("test_batch", test_size)]
    parts = {}
    for name, n in files:
        parts[name] = (rng.integers(0, 256, (n, 3072), dtype=np.uint8), rng.integers(0, 10, n).astype(np.int64))
    if "py" in layouts:
        d = os.path.join(root, "cifar-10-batches-py")
        os.makedirs(d, exist_ok=True)
        for name, (data, labels) in parts.items():
            with open(os.path.join(d, name), "wb") as fh:
                pickle.dump({"data": data, "labels": [int(v) for v in labels], "batch_label": name}, fh, protocol=2)
    if "bin" in layouts:
        d = os.path.join(root, "cifar-10-batches-bin")
        os.makedirs(d, exist_ok=True)
        for name, (data, labels) in parts.items():
            rec = np.concatenate([labels.astype(np.uint8)[:, None], data], axis=1)
            rec.tofile(os.path.join(d, name + ".bin"))
    tr = [parts[f"data_batch_{k + 1}"] for k in range(len(train_sizes))]
    return (np.concatenate([p[0] for p in tr]).reshape(-1, 3, 32, 32), np.concatenate([p[1] for p in tr]),
            parts["test_batch"][0].reshape(-1, 3, 32, 32), parts["test_batch"][1])


def c_hash4(a, b, c, d):
    """The C expression of the counter hash, on numpy uint32 scalars (wrapping arithmetic)."""
    u = np.uint32
    with np.errstate(over="ignore"):
        a, b, c, d = u(a & M32), u(b & M32), u(c & M32), u(d & M32)
        h = (a * u(0x9E3779B1)) ^ ((b + u(0x7F4A7C15)) * u(0x85EBCA77))
        h ^= (c + u(0x165667B1)) * u(0xC2B2AE3D)
        h = (h ^ (h >> u(15))) * u(0x2C1B3C6D)
        h ^= (d + u(0x27D4EB2F)) * u(0x9E3779B1)
        h = (h ^ (h >> u(13))) * u(0x297A2D39)
        return int(h ^ (h >> u(16)))


def oracle_draw(seed, epoch, index, pad, flip):
    h = c_hash4(seed, epoch, index, 0)
    dx = (((h & 0xFFFF) * (2 * pad + 1)) >> 16) - pad
    dy = (((h >> 16) * (2 * pad + 1)) >> 16) - pad
    return dx, dy, (c_hash4(seed, epoch, index, 1) >> 31) if flip else 0


def oracle_batch(src, labels, idx, rows, mean, std, pad=0, flip=False, seed=0, epoch=0, pad_target=-100):
    """Per-sample, per-pixel loops: ``(out [rows,C,32,32] f32, target [rows] i64, err)``."""
    N, C = src.shape[0], src.shape[1]
    scale = [np.float32(1.0 / (255.0 * s)) for s in std]
    shift = [np.float32(-m / s) for m, s in zip(mean, std)]
    out = np.zeros((rows, C, 32, 32), dtype=np.float32)
    tgt = np.full((rows,), pad_target, dtype=np.int64)
    err = 0
    for b in range(len(idx)):
        i = int(idx[b])
        if not 0 <= i < N:
            err = 1
            continue
        dx, dy, fl = oracle_draw(seed, epoch, i, pad, flip) if (pad or flip) else (0, 0, 0)
        if pad == 0:
            dx = dy = 0
        tgt[b] = labels[i]
        for c in range(C):
            for y in range(32):
                for x in range(32):
                    sy, sx = y + dy, (31 - x if fl else x) + dx
                    v = int(src[i, c, sy, sx]) if (0 <= sy < 32 and 0 <= sx < 32) else 0
                    out[b, c, y, x] = np.float32(float(v) * float(scale[c]) + float(shift[c]))
    return out, tgt, err
