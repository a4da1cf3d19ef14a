"""Boundary cases of the segmented reduce-copy (csrc/seg_block.h ``seg_reduce_block``) as ONE table,
and its reference: a numpy fp32 loop in chunk order.  Shared by the device test
(tests/test_kernels_gpu.py) and the CPU test that checks the reference against ``SegPlan``'s CPU
path (tests/test_seg_cases_cpu.py)."""
import itertools

import numpy as np
import torch

BAND = 64        # sentinel floats on either side of every dst
SENTINEL = -777.25
# around the float4 width and the 2048-element block; src / dst each starting 0 or 1 float past a
# 16-byte boundary (both 0: the float4 path and the float4 that crosses the end; otherwise the
# scalar path); chunks below, one over and two batches over the load batch of 8
NUMELS = (1, 3, 4, 5, 2047, 2048, 2049, 4097)
CHUNKS = (1, 2, 9, 17)
DIVS = (1.0, 3.0)
CASES = [dict(n=n, soff=so, doff=do, chunks=c, div=d)
         for n, so, do, c, d in itertools.product(NUMELS, (0, 1), (0, 1), CHUNKS, DIVS)]


def layout():
    """Element offsets: every case's src (``chunks`` slabs ``stride`` apart, stride % 4 == 0) and dst
    (a BAND on either side); returns (cases with src / dst / stride filled in, src total, dst total)."""
    out, s, d = [], 0, 0
    for c in CASES:
        stride = (c["n"] + 3) // 4 * 4 + 4
        src = s + c["soff"]
        s += c["chunks"] * stride + 4
        dst = d + BAND + c["doff"]
        d = (dst + c["n"] + BAND + 3) // 4 * 4
        out.append(dict(c, src=src, dst=dst, stride=stride))
    return out, s, d


def buffers(seed=0):
    cases, s_total, d_total = layout()
    rng = np.random.default_rng(seed)
    src = rng.standard_normal(s_total).astype(np.float32)
    dst = np.full(d_total, SENTINEL, dtype=np.float32)
    return cases, src, dst


def reference(cases, src, dst):
    """acc = src[0:n]; acc += src[c*stride : c*stride + n] in chunk order; / div: all fp32."""
    want = dst.copy()
    for c in cases:
        n, o, st = c["n"], c["src"], c["stride"]
        acc = src[o: o + n].copy()
        for k in range(1, c["chunks"]):
            acc = acc + src[o + k * st: o + k * st + n]
        if c["div"] != 1.0:
            acc = acc / np.float32(c["div"])
        assert acc.dtype == np.float32
        want[c["dst"]: c["dst"] + n] = acc
    return want


def specs(cases, src: torch.Tensor, dst: torch.Tensor):
    """The ``SegPlan`` specs over flat tensors ``src`` / ``dst`` (16-byte aligned bases)."""
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    out = []
    for c in cases:
        s, d = src[c["src"]:], dst[c["dst"]: c["dst"] + c["n"]]
        assert s.data_ptr() % 16 == 4 * c["soff"] and d.data_ptr() % 16 == 4 * c["doff"]
        out.append((s, d, c["chunks"], c["stride"], c["div"]))
    return out
