"""Test-side oracle of the mixup / CutMix batch rule (ops/image_batch.py: image_mix_batch), in plain
loops over numpy scalars, written independently of the torch twin: the base images come from
``image_rule.oracle_batch`` (one sample at a time) and the draws from ``c_hash4``."""
import math

import numpy as np

from .image_rule import c_hash4, oracle_batch

MODES = {"mixup": 1, "cutmix": 2, "mixup_cutmix": 3}


def oracle_mix_draw(seed, epoch, index, mode, mix_prob):
    """``(drawn, cut, lam (np.float32), box (x0, y0, x1, y1) or None)`` of one sample."""
    thr = int(mix_prob * (1 << 24))
    h3 = c_hash4(seed, epoch, index, 2)
    if not (h3 >> 8) < thr:
        return False, False, np.float32(1.0), None
    h4 = c_hash4(seed, epoch, index, 3)
    cut = MODES[mode] == 2 or (MODES[mode] == 3 and (h3 & 1) == 1)
    if not cut:
        return True, False, np.float32(h4 >> 8) * np.float32(2.0 ** -24), None
    h5 = c_hash4(seed, epoch, index, 4)
    side = math.isqrt(h4 >> 16) >> 3
    cx, cy = ((h5 & 0xFFFF) * 32) >> 16, ((h5 >> 16) * 32) >> 16
    x0, x1 = max(cx - (side >> 1), 0), min(cx - (side >> 1) + side, 32)
    y0, y1 = max(cy - (side >> 1), 0), min(cy - (side >> 1) + side, 32)
    lam = np.float32(1024 - (x1 - x0) * (y1 - y0)) / np.float32(1024.0)
    return True, True, lam, (x0, y0, x1, y1)


def oracle_mix_batch(src, labels, idx, rows, mean, std, mode, mix_prob, pad=0, flip=False, seed=0, epoch=0,
                     pad_target=-100, cache=None):
    """``(out [rows,C,32,32] f32, target, target_b [rows] i64, lam [rows] f32, err, kinds)``; ``kinds[b]`` is
    ``"pad"``, ``"self"`` (the centre row of an odd batch), ``"plain"``, ``"mixup"`` or ``"cutmix"``.
    ``cache`` (a dict, optional) keeps the base images between calls that share ``src``, ``mean`` / ``std``,
    ``pad``, ``flip``, ``seed`` and ``epoch``: they are computed once and left unchanged."""
    N, C = src.shape[0], src.shape[1]
    m = len(idx)
    out = np.zeros((rows, C, 32, 32), dtype=np.float32)
    tgt = np.full((rows,), pad_target, dtype=np.int64)
    tgt_b = np.full((rows,), pad_target, dtype=np.int64)
    lam = np.ones((rows,), dtype=np.float32)
    kinds = ["pad"] * rows
    err = 0

    cache = {} if cache is None else cache

    def base(i):  # image_batch's rule for one sample, with its own crop / flip draw
        if i not in cache:
            cache[i] = oracle_batch(src, labels, [i], 1, mean, std, pad, flip, seed, epoch, pad_target)[0][0]
        return cache[i]

    for b in range(m):
        i, j = int(idx[b]), int(idx[m - 1 - b])
        if not 0 <= i < N:
            err = 1
            continue
        if not 0 <= j < N:
            err = 1
        va = base(i)
        tgt[b] = tgt_b[b] = labels[i]
        out[b] = va
        kinds[b] = "self" if m - 1 - b == b else "plain"
        drawn, cut, l, box = oracle_mix_draw(seed, epoch, i, mode, mix_prob)
        if not drawn or m - 1 - b == b or not 0 <= j < N:
            continue
        vb = base(j)
        tgt_b[b] = labels[j]
        lam[b] = l
        kinds[b] = "cutmix" if cut else "mixup"
        for c in range(C):
            for y in range(32):
                for x in range(32):
                    if cut:
                        x0, y0, x1, y1 = box
                        out[b, c, y, x] = vb[c, y, x] if (x0 <= x < x1 and y0 <= y < y1) else va[c, y, x]
                    else:  # three fp32 roundings
                        p = np.float32(l * va[c, y, x])
                        q = np.float32((np.float32(1.0) - l) * vb[c, y, x])
                        out[b, c, y, x] = np.float32(p + q)
    return out, tgt, tgt_b, lam, err, kinds
