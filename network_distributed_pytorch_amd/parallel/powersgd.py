"""PowerSGD low-rank gradient compression with error feedback (Vogels et al., Alg. 1 + 2).

Two front-ends share one native execution plan:

* :class:`PowerSGDReducer` — API-compatible with the reference
  (ddp_powersgd_guide_cifar10/reducer.py:25-170):
  ``PowerSGDReducer(random_seed, device, n_power_iterations=0, reuse_query=True, rank=1)``
  and ``reduce(grad_in, grad_out, memory_out) -> bits``.
* :class:`PowerSGDOptimizer` — the reference training loop's whole "Algorithm 2" step
  (EF pack ``g + e``, compression, decompression, error memory, momentum, SGD update;
  ddp_powersgd_guide_cifar10/ddp_init.py:149-178) fused over flat parameter / gradient /
  error / momentum arenas: 4 kernel launches + 2 collectives per step (6 launches with
  ``NDP_FUSION_OFF=psgd_fin`` or above rank 16) instead of the reference's ~1.3k eager ops
  (SURVEY.md §2.6 launch-count evidence).

Per-step device pipeline (one launch each, all matrices at once):
  psgd_p  (P = (g+e) Q, e <- g+e; split-K sum of P and the rank-1 pack in the same launch)
  -> all_reduce([P | rank-1])      ->  psgd_orth (/N + batched MGS)
  -> psgd_q (Q = M^T P; split-K sum of Q in the same launch)
  -> all_reduce(Q)                 ->  psgd_update (out = P Q^T/N, e = M - out, momentum,
                                       x -= lr (out + m), warm-start Q, the rank-1 step)
Without the in-kernel finishes a seg_reduce launch follows psgd_p and psgd_q, and the rank-1
step is its own launch.
The P and rank-1 payloads share ONE collective (the reference issues them separately,
reducer.py:126,132); the byte count per step is unchanged.

Deliberate deviations: Q1 the Q-init RNG is a private generator seeded
exactly like the reference (``torch.manual_seed(rng.randint(1e9))`` per matrix) so the
values match but the global RNG is untouched; Q5 the unused 512 MiB ``precalc_numbers``
is not allocated (``rng_compat=True`` still advances the numpy stream the same way so Q
matches the reference bit-for-bit); Q6 models without <=1-D parameters are fine;
Q8 decompression writes parameter-shaped output directly.
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..ops import SegPlan, StateBlock, capturing, ext, gradfinish, taps, upload, upload_epoch
from ..ops.adamw import _twin_ as _adamw_twin_, adamw_scalars, check_adam_args
from ..ops.hyper import HyperState
from .comm import Communicator, n_bits
from .sync import GradSync
from ..knobs import fusion_on

__all__ = [
    "plan_layout",
    "Reducer",
    "PowerSGDReducer",
    "PowerSGDOptimizer",
    "orthogonalize",
    "powersgd_bytes_per_step",
]

_ALIGN = 16  # floats (64 B) — every high-rank arena slot starts 16-B aligned for float4


def plan_layout(shapes: Sequence[Tuple[int, int]], rank: int):
    """Pure-python P/Q layout (reference order, reducer.py:72-98)."""
    ranks, p_offs, q_offs = [], [], []
    p = q = 0
    for n, m in shapes:
        r = min(n, m, rank)
        ranks.append(r)
        p_offs.append(p)
        q_offs.append(q)
        p += n * r
        q += m * r
    return ranks, p_offs, q_offs, p, q


def powersgd_bytes_per_step(params: Sequence[torch.Tensor], rank: int) -> Dict[str, int]:
    """Bytes all-reduced per step with the reference's accounting."""
    shapes = [(p.shape[0], p.numel() // p.shape[0]) for p in params if p.dim() > 1]
    r1 = sum(p.numel() for p in params if p.dim() <= 1)
    _, _, _, pt, qt = plan_layout(shapes, rank)
    dense = sum(p.numel() for p in params)
    return {"p": 4 * pt, "rank1": 4 * r1, "q": 4 * qt, "total": 4 * (pt + r1 + qt), "dense": 4 * dense}


def orthogonalize(matrix: torch.Tensor, eps: float = 1e-8) -> torch.Tensor:
    """In-place modified Gram-Schmidt on the columns of ``matrix`` (reducer.py:180-191).

    Device tensors run the batched gfx950 kernel; CPU tensors use torch ops.
    """
    n, m = matrix.shape
    if matrix.is_cuda:
        assert matrix.dtype == torch.float32 and matrix.is_contiguous()
        X = ext()
        geom, items, n_items, max_rank = X.make_orth_geom([(int(n), int(m), 0)])
        scratch = torch.empty(2 * n_items * X.MAX_RANK, dtype=torch.float32, device=matrix.device)
        ctr = torch.zeros(2, dtype=torch.int64, device=matrix.device)
        X.psgd_orth(geom.to(matrix.device), items.to(matrix.device), matrix.view(-1), 1.0, float(eps),
                    int(max_rank), scratch, ctr)
        return matrix
    for i in range(m):
        col = matrix[:, i: i + 1]
        col /= torch.sqrt(torch.sum(col ** 2)) + eps
        if i + 1 < m:
            rest = matrix[:, i + 1:]
            rest -= torch.sum(col * rest, dim=0) * col
    return matrix


class Reducer:
    """Base reducer (reducer.py:6-23): rng, world size, device.

    ``rng_compat=True`` advances the numpy stream past the reference's 128M-sample
    ``precalc_numbers`` draw (without keeping it on the device, quirk Q5) so the Q-init
    seeds equal the reference's.
    """

    def __init__(self, random_seed: int, device, comm: Optional[Communicator] = None,
                 rng_compat: bool = False):
        self.rng = np.random.RandomState(random_seed)
        if rng_compat:
            left = 128 * 1024 * 1024
            while left > 0:
                k = min(left, 1 << 22)
                self.rng.randn(k)
                left -= k
        self.comm = comm if comm is not None else Communicator()
        self.n_workers = self.comm.world_size
        self.worker_rank = self.comm.rank  # quirk Q7: `rank` below means compression rank
        self.device = torch.device(device)

    def reduce(self, grad_in, grad_out, memory_out):
        """Return communicated bits."""
        raise NotImplementedError()


class _PlanBuffers:
    """Device/host buffers + native tables for one list of matrix shapes."""

    def __init__(self, shapes: List[Tuple[int, int]], rank: int, r1_numel: int, device: torch.device,
                 native: bool = True, supports: Optional[List[Tuple[int, int]]] = None):
        self.shapes = shapes
        self.rank = rank
        self.device = device
        self.ranks, self.p_offs, self.q_offs, self.p_total, self.q_total = plan_layout(shapes, rank)
        self.r1_numel = r1_numel
        self.max_rank = max(self.ranks) if self.ranks else 1
        f32 = dict(dtype=torch.float32, device=device)
        # comm buffer: [ P (sum n_i r_i) | rank-1 group ] -> ONE all-reduce
        self.comm_buf = torch.zeros(self.p_total + r1_numel, **f32)
        self.p_memory = self.comm_buf[: self.p_total]
        self.rank1_buf = self.comm_buf[self.p_total:]
        self.q_memory = torch.zeros(self.q_total, **f32)   # all-reduce payload for Q
        self.q_warm = torch.zeros(self.q_total, **f32)     # averaged Q = next step's query
        self.native = native and device.type == "cuda"
        # dead-tap compaction (ops/taps.py): (T, mask) of every matrix whose error memory and
        # momentum the plan keeps as [n, live columns], else None; compact_cols: their row length
        self.layout: List[Optional[Tuple[int, int]]] = [None] * len(shapes)
        self.compact_cols: List[int] = [m for _, m in shapes]
        if self.native:
            X = ext()
            d = self._build_tables(supports)
            self.p_part = torch.zeros(max(1, d["pp_total"]), **f32)
            self.q_part = torch.zeros(max(1, d["qp_total"]), **f32)
            self.orth_scratch = torch.zeros(max(1, 2 * d["n_orth_items"] * X.MAX_RANK), **f32)
            # 64-bit MGS barrier counters (never wrap) + the error word (low half of the last)
            self.orth_ctr = torch.zeros(len(shapes) + 1, dtype=torch.int64, device=device)
            nb = max(1, len(shapes)) * X.SIZEOF_MATGEOM
            self.geom = torch.zeros(nb, dtype=torch.uint8, device=device)
            self.ptrs = torch.zeros(nb, dtype=torch.uint8, device=device)
            self._bind_key = None
            self.q_seg = SegPlan(self.q_seg_specs(0, len(shapes)), device)
            # in-kernel split-K finish of P / Q (csrc/powersgd.hip PFin / QFin): monotonic arrival
            # counters, one per P row block / Q column block (zeroed once, never reset)
            self.p_ctr = torch.zeros(max(1, d["n_p_blocks"]), dtype=torch.int64, device=device)
            self._q_seg_fused = SegPlan(self.q_seg_specs(0, len(shapes), fused=True), device)
            self.fused = self.max_rank <= _LAZY_MAX_RANK and fusion_on("psgd_fin")

    def _build_tables(self, supports: Optional[List[Tuple[int, int]]]):
        """The native plan and its work-item tables for ``supports`` ((T, mask) per matrix, T = 0:
        none).  Only the Q / update items, the Q arrival counters and the geometry depend on them."""
        X = ext()
        device = self.device
        d = X.build_plan([(int(n), int(m)) for n, m in self.shapes], int(self.rank),
                         [(int(t), int(k)) for t, k in supports] if supports else [])
        assert d["p_total"] == self.p_total and d["q_total"] == self.q_total
        self._geom_host = d["geom"]
        self.p_items = d["p_items"].to(device)
        self.q_items = d["q_items"].to(device)
        self.u_items = d["u_items"].to(device)
        self.pp_offs, self.qp_offs = d["pp_offs"], d["qp_offs"]
        self.p_chunks, self.q_chunks = d["p_chunks"], d["q_chunks"]
        self.counts = {k: d[k] for k in ("n_p_items", "n_q_items", "n_u_items", "n_orth_items", "pp_total",
                                         "qp_total")}
        self.item_start = {k: d[k + "_item_start"] for k in ("p", "q", "u", "orth")}
        self.orth_items = d["orth_items"].to(device)
        self.p_cols = int(d["p_cols"])  # columns per P item
        self.q_ctr = torch.zeros(max(1, d["n_q_blocks"]), dtype=torch.int64, device=device)
        self.layout = [tuple(supports[i]) if t else None for i, t in enumerate(d["tap_T"])]
        self.compact_cols = [int(c) for c in d["compact_cols"]]
        return d

    def replan(self, supports: Optional[List[Tuple[int, int]]]):
        """Rebuild the tables for new supports (never while capturing: the tables are new tensors).
        The Q kernel never writes a dead Q row, so the Q sums and partials start from zero."""
        assert self.native and not capturing()
        self._build_tables(supports)
        self.q_memory.zero_()
        self.q_part.zero_()
        self._bind_key = None

    def vec_flag(self, i: int, row: Sequence[int]) -> int:
        """MatGeom.vec of matrix ``i`` bound to the MatPtrs ``row``: float4 eligibility; for a
        compacted matrix bit 0 covers the full-width arrays (grad, x) and bit 1 the compact ones."""
        if self.layout[i] is None:
            return _vec_ok(self.shapes[i][1], row)
        return (_vec_ok(self.shapes[i][1], (row[0], row[6], row[7]))
                | _vec_ok(self.compact_cols[i], (row[1], row[2], row[5])) << 1)

    # -- per-matrix-range views (a PowerSGD overlap group = matrices [lo, hi)) ----------------
    def p_seg_specs(self, lo: int = 0, hi: Optional[int] = None):
        hi = len(self.shapes) if hi is None else hi
        return [(self.p_part[self.pp_offs[i]:], self.p_memory[self.p_offs[i]: self.p_offs[i] + n * r],
                 self.p_chunks[i], n * r, 1.0)
                for i, ((n, m), r) in enumerate(zip(self.shapes, self.ranks)) if lo <= i < hi]

    def q_seg_specs(self, lo: int, hi: int, fused: bool = False):
        """Split-K sums of Q for matrices [lo, hi); ``fused``: only those the Q kernel does not
        finish itself (more than ``Q_FIN_MAX`` row chunks)."""
        return [(self.q_part[self.qp_offs[i]:], self.q_memory[self.q_offs[i]: self.q_offs[i] + m * r],
                 self.q_chunks[i], m * r, 1.0)
                for i, ((n, m), r) in enumerate(zip(self.shapes, self.ranks))
                if lo <= i < hi and (not fused or self.q_chunks[i] > Q_FIN_MAX)]

    def items(self, kind: str, lo: int, hi: int) -> torch.Tensor:
        """Byte slice of a work-item table covering matrices [lo, hi)."""
        size = {"p": 32, "q": 32, "u": 16, "orth": 32}[kind]  # sizeof PItem / QItem / UItem / OrthItem
        table = {"p": self.p_items, "q": self.q_items, "u": self.u_items, "orth": self.orth_items}[kind]
        st = self.item_start[kind]
        return table[st[lo] * size: st[hi] * size]

    def p_range(self, lo: int, hi: int) -> Tuple[int, int]:
        end = self.p_offs[hi - 1] + self.shapes[hi - 1][0] * self.ranks[hi - 1]
        return self.p_offs[lo], end

    def q_range(self, lo: int, hi: int) -> Tuple[int, int]:
        end = self.q_offs[hi - 1] + self.shapes[hi - 1][1] * self.ranks[hi - 1]
        return self.q_offs[lo], end

    def run_p(self, items: torch.Tensor, fuse_ef: bool, p_prev: Optional[torch.Tensor] = None,
              seg: Optional[SegPlan] = None, p_seg: Optional[SegPlan] = None):
        """P = M Q for the matrices of ``items`` (+ the rank-1 pack ``seg``): one launch when the
        split-K sums run in-kernel (``fused``), else the kernel + ``p_seg`` (sums and pack)."""
        X = ext()
        if not self.fused:
            if self.shapes:
                X.psgd_p(self.geom, self.ptrs, items, self.q_warm, self.p_part, fuse_ef, self.max_rank, p_prev,
                         p_cols=self.p_cols, err=self.orth_ctr)
            if p_seg is not None:
                p_seg.run()
            return
        t = seg.table() if seg is not None else None
        if not self.shapes and t is None:
            return
        kw = dict(seg_entries=t[0], seg_prefix=t[1], seg_n=t[2], seg_blocks=t[3]) if t is not None else {}
        X.psgd_p(self.geom, self.ptrs, items, self.q_warm, self.p_part, fuse_ef, self.max_rank, p_prev,
                 p_out=self.comm_buf, p_ctr=self.p_ctr, p_cols=self.p_cols, err=self.orth_ctr, **kw)

    def run_q(self, items: torch.Tensor, q_seg: SegPlan, q_seg_fused: Optional[SegPlan] = None):
        """Q = M^T P-hat into q_memory: split-K sums in-kernel when ``fused`` (+ ``q_seg_fused`` for
        the matrices with more than Q_FIN_MAX row chunks), else + ``q_seg``."""
        X = ext()
        if self.fused:
            X.psgd_q(self.geom, self.ptrs, items, self.comm_buf, self.q_part, self.max_rank,
                     q_out=self.q_memory, q_ctr=self.q_ctr, q_fin_max=Q_FIN_MAX)
            (self._q_seg_fused if q_seg_fused is None else q_seg_fused).run()
        else:
            X.psgd_q(self.geom, self.ptrs, items, self.comm_buf, self.q_part, self.max_rank)
            q_seg.run()

    def orth(self, p_div: float, eps: float, items: Optional[torch.Tensor] = None, max_spins: int = -1):
        """P-hat = MGS(P / p_div) for every matrix (or a group's item slice), one launch."""
        ext().psgd_orth(self.geom, self.orth_items if items is None else items, self.comm_buf, p_div, eps,
                        self.max_rank, self.orth_scratch, self.orth_ctr, self.counts["n_orth_items"], max_spins)

    def orth_error(self) -> int:
        """The sticky device error word (host sync): bit 0 = a cross-workgroup barrier of the MGS
        kernel timed out, bit 1 = a gradient was nonzero in a conv tap recorded as dead."""
        return int(self.orth_ctr[-1].item())

    def check_orth(self):
        err = self.orth_error() if self.native else 0
        if err & 1:
            raise RuntimeError("PowerSGD orthogonalisation: a cross-workgroup barrier timed out; P-hat "
                               "was poisoned with NaN (co-residency violated)")
        if err & 2:
            raise RuntimeError("PowerSGD dead-tap compaction: a gradient was nonzero in a conv tap recorded as "
                               "never seeing a real pixel; its error memory and momentum were dropped "
                               "(NDP_FUSION_OFF=dead_taps keeps the full layout)")

    def bind(self, rows: List[List[int]], vec: List[int]) -> bool:
        """Point the grouped kernels at new tensors; returns True if the tables changed."""
        key = (upload_epoch(), tuple(map(tuple, rows)), tuple(vec))
        if key == self._bind_key:
            return False
        X = ext()
        upload(self.geom, X.patch_geom_vec(self._geom_host, vec))
        upload(self.ptrs, X.make_mat_ptrs(rows))
        self._bind_key = key
        return True

    def bind_range(self, lo: int, rows: List[List[int]], vec: List[int]):
        """Upload geometry + pointer rows of matrices [lo, lo + len(rows)) only."""
        X = ext()
        sz = X.SIZEOF_MATGEOM
        hi = lo + len(rows)
        geom = self._geom_host[lo * sz: hi * sz].clone()
        gi = geom.view(torch.int32).view(hi - lo, sz // 4)
        gi[:, 3] = torch.tensor(vec, dtype=torch.int32)  # MatGeom.vec
        upload(self.geom[lo * sz: hi * sz], geom)
        upload(self.ptrs[lo * X.SIZEOF_MATPTRS: hi * X.SIZEOF_MATPTRS], X.make_mat_ptrs(rows))

    def p_view(self, i):
        n, _ = self.shapes[i]
        return self.p_memory[self.p_offs[i]: self.p_offs[i] + n * self.ranks[i]].view(n, self.ranks[i])

    def q_view(self, i, buf=None):
        _, m = self.shapes[i]
        buf = self.q_warm if buf is None else buf
        return buf[self.q_offs[i]: self.q_offs[i] + m * self.ranks[i]].view(m, self.ranks[i])


def _vec_ok(m: int, ptrs: Sequence[int]) -> int:
    return int(m % 4 == 0 and all(p % 16 == 0 for p in ptrs if p))


class PowerSGDReducer(Reducer):
    """Rank-r PowerSGD with warm-started Q and error feedback (reducer.py:25-170)."""

    def __init__(self, random_seed, device, n_power_iterations=0, reuse_query=True, rank=1,
                 comm: Optional[Communicator] = None, rng_compat: bool = False, eps: float = 1e-8):
        super().__init__(random_seed, device, comm=comm, rng_compat=rng_compat)
        assert n_power_iterations == 0
        self.rank = rank
        self.reuse_query = reuse_query
        self.eps = eps
        self._buf: Optional[_PlanBuffers] = None
        self.p_memory = None
        self.q_memory = None
        self._bind_key = None
        self._p_seg = None
        self._r1_unpack = None

    def _set_random(self, q: torch.Tensor):
        # reducer.py:36-38 with a private generator (quirk Q1): same seed stream, same values
        seed = int(self.rng.randint(1_000_000_000))
        gen = torch.Generator(device=q.device)
        gen.manual_seed(seed)
        q.copy_(torch.randn(*q.shape, generator=gen, device=q.device, dtype=q.dtype))

    def _init_queries(self, first: bool):
        if self.reuse_query and not first:
            return
        for i in range(len(self._buf.shapes)):
            self._set_random(self._buf.q_view(i))

    # ------------------------------------------------------------------------------------
    def reduce_torch(self, grad_in, grad_out, memory_out):
        """Eager-PyTorch reference-semantics path on any device (comparison arm)."""
        return self.reduce(grad_in, grad_out, memory_out, force_torch=True)

    def reduce(self, grad_in, grad_out, memory_out, force_torch: bool = False):
        rank1 = [(t, o, m) for t, o, m in zip(grad_in, grad_out, memory_out) if t.ndimension() <= 1]
        high = [(t, o, m) for t, o, m in zip(grad_in, grad_out, memory_out) if t.ndimension() > 1]
        first = self._buf is None
        if first:  # sized once, on the first call (quirk Q9 kept)
            shapes = [(t.shape[0], t.numel() // t.shape[0]) for t, _, _ in high]
            self._buf = _PlanBuffers(shapes, self.rank, sum(t.numel() for t, _, _ in rank1), self.device,
                                     native=not force_torch)
            self.p_memory = self._buf.p_memory
            self.q_memory = self._buf.q_memory
        B = self._buf
        self._init_queries(first)
        N = self.n_workers
        if B.native and not force_torch:
            assert all(t.is_cuda for t, _, _ in high + rank1), "mixed host/device tensors"
            self._reduce_native(high, rank1, N)
        else:
            self._reduce_torch(high, rank1, N)
        return n_bits(B.p_memory) + n_bits(B.rank1_buf) + n_bits(B.q_memory)

    # -- device path: 4 launches (6 without the in-kernel split-K finishes) + 2 collectives --
    def _bind(self, high, rank1):
        B = self._buf
        key = tuple(x.data_ptr() for trip in high + rank1 for x in trip)
        if key == self._bind_key:
            return
        rows, vec = [], []
        for (t, o, m), (n, mm) in zip(high, B.shapes):
            assert t.is_contiguous() and o.is_contiguous() and m.is_contiguous()
            row = [t.data_ptr(), 0, t.data_ptr(), o.data_ptr(), m.data_ptr(), 0, 0, 0]
            rows.append(row)
            vec.append(_vec_ok(mm, row))
        B.bind(rows, vec)
        specs = [] if B.fused else B.p_seg_specs()  # fused: the P launch sums its slabs itself
        off = 0
        for t, _, _ in rank1:
            specs.append((t.reshape(-1), B.rank1_buf[off: off + t.numel()], 1, 0, 1.0))
            off += t.numel()
        off = 0
        unpack = []
        for _, o, _ in rank1:
            unpack.append((B.rank1_buf[off: off + o.numel()], o.view(-1), 1, 0, float(self.n_workers)))
            off += o.numel()
        if self._p_seg is None:
            self._p_seg = SegPlan(specs, B.device)
            self._r1_unpack = SegPlan(unpack, B.device)
        else:
            self._p_seg.set(specs)
            self._r1_unpack.set(unpack)
        self._bind_key = key

    def _reduce_native(self, high, rank1, N):
        B = self._buf
        X = ext()
        self._bind(high, rank1)
        B.run_p(B.p_items, False, seg=self._p_seg, p_seg=self._p_seg)   # P (+ split-K sum) + rank-1 pack
        self.comm.all_reduce(B.comm_buf)                    # reducer.py:126 + :132 fused
        if B.shapes:
            B.orth(float(N), self.eps)
            B.run_q(B.q_items, B.q_seg)
            self.comm.all_reduce(B.q_memory)                # reducer.py:145
            X.psgd_update(B.geom, B.ptrs, B.u_items, B.comm_buf, B.q_memory, float(N),
                          B.q_warm, 0, 0.0, 0.0, B.max_rank)
        self._r1_unpack.run()                               # reducer.py:166-168

    # -- CPU / reference-semantics path --------------------------------------------------
    def _reduce_torch(self, high, rank1, N):
        B = self._buf
        for i, (t, _, _) in enumerate(high):
            torch.matmul(t.view(t.shape[0], -1), B.q_view(i), out=B.p_view(i))
        off = 0
        for t, _, _ in rank1:
            B.rank1_buf[off: off + t.numel()].copy_(t.reshape(-1))
            off += t.numel()
        self.comm.all_reduce(B.comm_buf)
        B.p_memory.div_(N)
        for i in range(len(high)):
            orthogonalize(B.p_view(i), self.eps)
        for i, (t, _, _) in enumerate(high):
            torch.matmul(t.view(t.shape[0], -1).t(), B.p_view(i), out=B.q_view(i, B.q_memory))
        self.comm.all_reduce(B.q_memory)
        B.q_memory.div_(N)
        B.q_warm.copy_(B.q_memory)
        for i, (t, o, m) in enumerate(high):
            out = torch.matmul(B.p_view(i), B.q_view(i).t())
            o.copy_(out.view_as(o))
            m.copy_(t - o)
        off = 0
        for _, o, _ in rank1:
            o.copy_((B.rank1_buf[off: off + o.numel()] / N).view_as(o))
            off += o.numel()


_LAZY_MAX_RANK = 16  # csrc/ndp_kernels.h kUWideMaxRank: the wide P / update kernels
# Q split-K chunks the Q kernel's last arriver sums itself; taller matrices (DistilBERT's 30522-row
# embedding: 120 chunks) keep a seg_reduce launch, which spreads that sum over the whole device
Q_FIN_MAX = int(os.environ.get("NDP_QFIN_MAX", "32"))


class _Group:
    """One overlap group: high-rank matrices [lo, hi) (contiguous in parameter order, so
    their P / Q payloads are contiguous slices of the reference-order buffers)."""

    def __init__(self, idx: int, lo: int, hi: int, params: List[torch.nn.Parameter]):
        self.idx, self.lo, self.hi = idx, lo, hi
        self.params = params
        self.numel = sum(p.numel() for p in params)
        self.ready = 0
        self.launched = False
        self.key = None
        self.p_seg: Optional[SegPlan] = None
        self.q_seg: Optional[SegPlan] = None
        self.q_seg_fused: Optional[SegPlan] = None


class PowerSGDOptimizer(HyperState, GradSync):
    """Fused EF-SGD-with-momentum PowerSGD step (ddp_init.py:121-178) over flat arenas.

    Parameters are re-pointed into a flat parameter arena ``x`` (every high-rank slot 64-B
    aligned, the <=1-D group contiguous at the end) with matching error-memory ``e`` and
    momentum ``m`` arenas.  Gradients stay wherever autograd produced them (no in-place
    accumulation into a preset ``.grad`` — that costs one extra add kernel per parameter);
    the grouped kernels reach them through a device pointer table that is re-uploaded only
    when an address changes (hipGraph-capture safe).  ``step()`` returns the bits
    communicated (reducer.py:170).

    **Overlap with backward** (``overlap=True``, the default on a device with a
    stream-ordered data plane — native RCCL, or nothing to communicate).  The high-rank
    matrices are cut, in backward order, into ``groups`` contiguous groups.  A
    post-accumulate-grad hook launches a group's whole pipeline on the communicator's side
    stream as soon as its last gradient lands, in group order on every rank:

        psgd_p -> split-K sum -> all_reduce(P_g) -> MGS -> psgd_q -> split-K sum
               -> all_reduce(Q_g) -> fused decompress / EF / momentum / SGD update

    so compression, both collectives and the update of the late layers run while backward
    is still computing the early layers.  ``step()`` launches what is left (the rank-1
    group: pack, all-reduce, momentum/SGD) and joins the side stream.  Per-matrix work
    items, split-K slab order and the MGS reduction order are exactly those of the serial
    path, so the result is bitwise identical to ``overlap=False`` (tests/test_overlap_gpu.py);
    the byte count is unchanged, the collective count becomes 2 * groups + 1.

    ``write_grad=True`` also leaves ``p.grad = out + m`` exactly like the reference loop
    (ddp_init.py:172); it costs one extra write pass and is off by default.

    **Lazy error feedback** (native, rank <= 16; ``NDP_FUSION_OFF=lazy_ef`` turns it off): the
    update pass does not store ``e = M - P Q^T`` — it would read ``M`` back only for that
    store, 2 of its 6 arena passes.  The arena keeps ``M`` and ``p_prev`` keeps the step's
    P-hat; the next P pass forms ``e`` element by element with the update kernel's exact
    arithmetic (csrc/powersgd.hip), so every step is bitwise the eager formula's.  :attr:`e`
    (and ``state_dict``) materialise the true error memory first.

    **Hyper-parameter block** (:meth:`set_hyper`): the native optimiser owns a 16-byte device tensor
    ``hyper = [lr, weight_decay, 0, 0]`` (ops/hyper.py, csrc/hyper.h).  Once :meth:`set_hyper` has
    been called (or with ``weight_decay != 0``) the update kernels read both values from it, so a
    schedule reaches a captured step: the block is overwritten between graph replays.  An
    optimiser that never calls it passes ``lr`` by value as before, bitwise the same step.
    ``weight_decay`` is L2 on every parameter, ``d = out + wd x`` after decompression; it never
    enters the error memory, P, Q or the all-reduced bytes.  Dead taps acquire momentum under it,
    so with ``weight_decay != 0`` every matrix keeps the full layout.

    **Gradient clipping** (``max_grad_norm > 0``; ops/gradclip.py, csrc/gradclip.hip): ``phase_p``
    clips every parameter's gradient, the <=1-D group included, by their global L2 norm in two
    launches before anything reads them, so the whole-step and the piecewise graph contain the
    clip.  ``inf`` measures the norm and never scales.  With more than one rank, each rank clips
    its OWN gradient by its OWN norm before it enters ``M = g + e``: the error feedback sees the
    clipped gradient, and :meth:`clip_stats` reports a rank-local norm.  The norm needs every
    gradient, so the per-group pipelines cannot start during backward: ``overlap=None`` resolves
    to ``False`` and ``overlap=True`` / ``set_overlap(True)`` raise.

    **AdamW** (``optimizer="adamw"`` with ``betas``, ``eps_adam``, ``decay_1d``; ``eps`` is the
    orthogonaliser's): the update launches apply the AdamW rule of ops/adamw.py to the decompressed
    value in the pass that decompresses (csrc/powersgd.hip ``psgd_update_adam_wide_kernel``, ``g := out``,
    ``div = 1``; the <=1-D group with ``g := rank1 / N``), in the place of momentum SGD; ``momentum`` is
    ignored, ``weight_decay`` is the decoupled decay (every matrix; the <=1-D group with ``decay_1d``),
    ``write_grad`` leaves ``p.grad = out``, the decompressed, averaged gradient.  Error memory, P, Q and
    the wire are untouched.  The moment arena is ``[m | v]`` in one tensor, the 16-byte block
    ``{b1pow, b2pow, steps}`` (:meth:`adam_stats`) starts as ``{1, 1, 0}``, and the hyper block is
    always read.  A step may hold several update launches (one per overlap group, then the rank-1
    one): all read the block as it was before the step and only the last one advances it.  Scope:
    plan rank <= 16 (above it the constructor raises) and the full layout only (no dead-tap
    compaction, whatever the decay).  With ``optimizer="sgd"`` nothing of this is allocated, launched or
    stored.
    """

    _arm = "PowerSGD"

    def __init__(self, params, lr: float, momentum: float = 0.9, rank: int = 4,
                 random_seed: int = 714, reuse_query: bool = True,
                 comm: Optional[Communicator] = None, write_grad: bool = False,
                 broadcast_params: bool = True, rng_compat: bool = False, eps: float = 1e-8,
                 native: Optional[bool] = None, overlap: Optional[bool] = None, groups: Optional[int] = None,
                 weight_decay: float = 0.0, max_grad_norm: float = 0.0, optimizer: str = "sgd",
                 betas=(0.9, 0.999), eps_adam: float = 1e-8, decay_1d: bool = True):
        self.params: List[torch.nn.Parameter] = [p for p in params]
        assert self.params, "no parameters"
        if optimizer not in ("sgd", "adamw"):
            raise ValueError(f"PowerSGD: unknown optimizer {optimizer!r} (sgd, adamw)")
        self.optimizer = optimizer
        self.adam = optimizer == "adamw"
        if self.adam:
            self.beta1, self.beta2, self.eps_adam = check_adam_args(betas, eps_adam)
            self.decay_1d = bool(decay_1d)
        assert weight_decay >= 0, "weight_decay >= 0"
        if max_grad_norm > 0 and overlap:
            raise ValueError("PowerSGD: overlap=True cannot be combined with max_grad_norm > 0 (the global "
                             "norm needs every gradient before the first group's pipeline may start)")
        self.momentum = float(momentum)
        self.rank = int(rank)
        self.reuse_query = reuse_query
        self.write_grad = write_grad
        self.eps = eps
        self.comm = comm if comm is not None else Communicator()
        self.device = self.params[0].device
        self.rng = np.random.RandomState(random_seed)
        if rng_compat:
            left = 128 * 1024 * 1024
            while left > 0:
                k = min(left, 1 << 22)
                self.rng.randn(k)
                left -= k
        self.step_count = 0
        self.bits_communicated = 0
        self._q_ready = False
        self.orth_max_spins = -1  # < 0: kernel default (debug / tests may lower it)

        hi = [p for p in self.params if p.dim() > 1]
        r1 = [p for p in self.params if p.dim() <= 1]
        self.high, self.rank1 = hi, r1
        offs, o = {}, 0
        for p in hi:
            offs[id(p)] = o
            o += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self.r1_start = o
        for p in r1:
            offs[id(p)] = o
            o += p.numel()
        self.arena_numel = o
        f32 = dict(dtype=torch.float32, device=self.device)
        self.x = torch.zeros(o, **f32)
        self._e = torch.zeros(o, **f32)
        if self.adam:  # [m | v] in one tensor: v lies _v_delta elements behind m, as far past 16 bytes
            self._v_delta = (o + _ALIGN - 1) // _ALIGN * _ALIGN
            self._moments = torch.zeros(2 * self._v_delta, **f32)
            self._m = self._moments[:o]
            self._v = self._moments[self._v_delta: self._v_delta + o]
        else:
            self._m = torch.zeros(o, **f32)
        self.offsets = offs
        with torch.no_grad():
            for p in self.params:
                s = offs[id(p)]
                view = self.x[s: s + p.numel()].view_as(p)
                view.copy_(p.data)
                p.data = view
                p.grad = None
        if broadcast_params:  # quirks Q3/Q4: replicas start identical (one flat broadcast)
            self.comm.broadcast(self.x, src=0)

        shapes = [(p.shape[0], p.numel() // p.shape[0]) for p in hi]
        self.r1_numel = o - self.r1_start
        self.r1_upd = torch.zeros(self.r1_numel if write_grad else 0, **f32)
        self.buf = _PlanBuffers(shapes, self.rank, self.r1_numel, self.device, native=native is not False)
        self.native = self.buf.native
        if self.adam and self.buf.max_rank > _LAZY_MAX_RANK:
            raise ValueError(f"PowerSGD with optimizer='adamw': plan rank {self.buf.max_rank} > {_LAZY_MAX_RANK}; the "
                             "AdamW update exists for the wide update tile only (rank <= 16)")
        # device block [lr, weight_decay, 0, 0], allocated before any capture; the kernels read it
        # once set_hyper() was called or a decay is on, else lr goes by value (see set_hyper); the
        # AdamW launches have no by-value lr: always on
        self._init_hyper(float(lr), float(weight_decay), block=self.native, on=True if self.adam else None)
        if self.adam:
            # the AdamBlock and, on a device, the arrival tickets of the largest update launch (the
            # fused one: every update item + 512 rank-1 blocks; the rank-1 launch alone: 1024)
            self.adam_state = StateBlock(self.device, ("b1pow", "b2pow", "steps"), (1.0, 1.0, 0))
            if self.native:
                X = ext()
                self._adam_ctr = torch.zeros(X.arrive_ctr_words(self.buf.counts["n_u_items"] + 1024),
                                             dtype=torch.int32, device=self.device)
        # dead-tap compaction (ops/taps.py; NDP_FUSION_OFF=dead_taps): the support version the plan
        # was last compared with (None: compare at the next step)
        self.dead_taps = self.native and bool(shapes) and fusion_on("dead_taps")
        self._taps_seen: Optional[int] = None
        # needs the warm-start Q of the next P pass to BE the update's Qs (reuse_query)
        self.lazy_ef = (self.native and bool(shapes) and self.buf.max_rank <= _LAZY_MAX_RANK and reuse_query
                        and fusion_on("lazy_ef"))
        self._lazy_pending = False  # an update ran since e was last materialised
        # P-hat of the last update (lazy error feedback); zero = no pending correction
        self.p_prev = torch.zeros(self.buf.p_total if self.lazy_ef else 0, **f32)
        self._p_seg = SegPlan([], self.device, capacity=len(shapes) + len(r1) + 1) if self.native else None
        self._r1_out = SegPlan([], self.device, capacity=len(r1) + 1) if self.native else None
        self._r1_pack = SegPlan([], self.device, capacity=len(r1) + 1) if self.native else None
        self._grad_key = None
        self._r1_key = None
        # global-norm clip of this rank's gradients (ops/gradclip.py): table, partials and the
        # {norm, coef, clipped, steps} block exist before any capture
        self._init_clip(max_grad_norm, self.device, capacity=len(self.params),
                        blocks=sum((p.numel() + 2047) // 2048 for p in self.params))
        if self.clip is not None:
            overlap = False  # overlap=None resolves to the serial step

        # default: overlap when a step has wire time to hide (N > 1 or link emulation)
        want = overlap if overlap is not None else (os.environ.get("NDP_PSGD_OVERLAP", "1") != "0"
                                                    and self.comm.has_traffic)
        self.overlap = bool(want) and self.native and self.comm.stream_ordered and bool(hi)
        if overlap and not self.overlap:
            raise ValueError("overlap=True needs device tensors, the native extension and a stream-ordered "
                             "communicator (native RCCL or world size 1)")
        self.groups: List[_Group] = []
        self._group_of = {}
        self._hooks = []
        self._next_group = 0
        if self.overlap:
            n_groups = groups if groups is not None else int(os.environ.get("NDP_PSGD_GROUPS", "4"))
            self._build_groups(max(1, n_groups))
            for p in self.params:
                self._hooks.append(p.register_post_accumulate_grad_hook(self._on_grad))

    # -- overlap groups ------------------------------------------------------------------------
    def _build_groups(self, n_groups: int):
        """Cut the high-rank matrices, in backward (reverse parameter) order, into groups of
        about total/n_groups elements; the last group to be produced (the first layers) is
        whatever is left, so the exposed post-backward tail stays small."""
        total = sum(p.numel() for p in self.high)
        target = total / n_groups
        bounds = []  # (lo, hi) in forward index space, built from the back
        hi_idx = len(self.high)
        acc = 0
        for i in range(len(self.high) - 1, -1, -1):
            acc += self.high[i].numel()
            if acc >= target and len(bounds) < n_groups - 1 and i > 0:
                bounds.append((i, hi_idx))
                hi_idx, acc = i, 0
        bounds.append((0, hi_idx))
        for gi, (lo, hi) in enumerate(bounds):
            g = _Group(gi, lo, hi, self.high[lo:hi])
            g.p_seg = SegPlan([], self.device, capacity=hi - lo + 1)
            g.q_seg = SegPlan(self.buf.q_seg_specs(lo, hi), self.device)
            if self.buf.native:
                g.q_seg_fused = SegPlan(self.buf.q_seg_specs(lo, hi, fused=True), self.device)
            self.groups.append(g)
            for p in g.params:
                self._group_of[id(p)] = g

    def _on_grad(self, p):
        if not self.overlap:
            return
        g = self._group_of.get(id(p))
        if g is None:
            return  # rank-1 parameters are handled in step()
        g.ready += 1
        # launch in group order on every rank (identical collective sequence everywhere)
        while self._next_group < len(self.groups):
            nxt = self.groups[self._next_group]
            if nxt.launched or nxt.ready < len(nxt.params):
                break
            self._launch_group(nxt)
            self._next_group += 1

    def _bind_group(self, g: _Group):
        B = self.buf
        grads = [p.grad for p in g.params]
        key = (upload_epoch(),) + tuple(t.data_ptr() for t in grads)
        if key == g.key:
            return
        rows, vec = [], []
        for p, gr, (n, m) in zip(g.params, grads, B.shapes[g.lo:g.hi]):
            assert gr.is_contiguous() and gr.dtype == torch.float32, "PowerSGD needs dense fp32 grads"
            s = self.offsets[id(p)]
            e, mo, x = (t[s:].data_ptr() for t in (self._e, self._m, self.x))
            row = [gr.data_ptr(), e, e, 0, 0, mo, x, gr.data_ptr()]
            rows.append(row)
            vec.append(B.vec_flag(g.lo + len(vec), row))
        B.bind_range(g.lo, rows, vec)
        g.p_seg.set(B.p_seg_specs(g.lo, g.hi))
        g.key = key

    @torch.no_grad()
    def _launch_group(self, g: _Group):
        gradfinish.flush()  # deferred conv grad-W sums / folds of the layers done so far
        if g.idx == 0:  # the step's first reducer launch (groups launch in order)
            self._sync_supports()
        B = self.buf
        X = ext()
        N = self.comm.world_size
        self._ensure_queries()
        for p in g.params:
            if p.grad is None:  # parameter unused this step: zero gradient
                p.grad = torch.zeros_like(p)
        self._bind_group(g)  # table uploads on the compute stream, before the fork
        p0, p1 = B.p_range(g.lo, g.hi)
        q0, q1 = B.q_range(g.lo, g.hi)
        mode, lr, mom, spins = 2 if self.write_grad else 1, self.lr, self.momentum, self.orth_max_spins
        hy = self._hyper_arg()

        pp = self.p_prev if self.lazy_ef else None

        def pipeline():
            B.run_p(B.items("p", g.lo, g.hi), True, pp, p_seg=g.p_seg)
            self.comm.all_reduce(B.comm_buf[p0:p1])                       # reducer.py:126 (group g)
            B.orth(float(N), self.eps, B.items("orth", g.lo, g.hi), spins)
            B.run_q(B.items("q", g.lo, g.hi), g.q_seg, g.q_seg_fused)
            self.comm.all_reduce(B.q_memory[q0:q1])                       # reducer.py:145 (group g)
            if self.adam:  # the block advances in the step's last update launch: the rank-1 one if any
                self._update_adam(B.items("u", g.lo, g.hi), N, pp, hy,
                                  advance=g is self.groups[-1] and not self.r1_numel)
                return
            X.psgd_update(B.geom, B.ptrs, B.items("u", g.lo, g.hi), B.comm_buf, B.q_memory, float(N),
                          B.q_warm, mode, lr, mom, B.max_rank, pp, hyper=hy)
        self.comm.side_launch(pipeline)
        g.launched = True

    def _finish_overlapped(self):
        """After backward: launch groups whose hooks did not fire (unused parameters / hooks
        bypassed), run the rank-1 group on the side stream, join."""
        for g in self.groups[self._next_group:]:
            if not g.launched:
                self._launch_group(g)
        self._next_group = len(self.groups)
        B = self.buf
        N = self.comm.world_size
        if self.r1_numel:
            grads = []
            for p in self.rank1:
                if p.grad is None:
                    p.grad = torch.zeros_like(p)
                grads.append(p.grad)
            key = (upload_epoch(),) + tuple(t.data_ptr() for t in grads)
            if key != self._r1_key:
                specs, outs = [], []
                for p, gr in zip(self.rank1, grads):
                    s = self.offsets[id(p)] - self.r1_start
                    specs.append((gr.view(-1), B.rank1_buf[s: s + p.numel()], 1, 0, 1.0))
                    if self.write_grad:
                        outs.append((self.r1_upd[s: s + p.numel()], gr.view(-1), 1, 0, 1.0))
                self._r1_pack.set(specs)
                self._r1_out.set(outs)
                self._r1_key = key
            r1 = slice(self.r1_start, self.arena_numel)
            lr, mom, hy = self.lr, self.momentum, self._hyper_arg()

            def rank1():
                self._r1_pack.run()
                self.comm.all_reduce(B.rank1_buf)                           # reducer.py:132
                if self.adam:
                    self._rank1_adam(N, hy, advance=True)
                else:
                    ext().rank1_step(B.rank1_buf, float(N), self._m[r1], self.x[r1],
                                     self.r1_upd if self.write_grad else None, lr, mom, hyper=hy)
                if self.write_grad:
                    self._r1_out.run()
                self._after_update()  # the EMA: behind the step's last update launch, same side item
            self.comm.side_launch(rank1)
        elif self.ema is not None:
            self.comm.side_launch(self._after_update)
        self.comm.side_join()

    # -- AdamW launches ------------------------------------------------------------------------
    def _adam_kw(self, advance: bool, hyper):
        """The Adam arguments of one update launch; ``advance``: it is the step's last one."""
        return dict(hyper=hyper, block=self.adam_state.dev, ctr=self._adam_ctr, moments=self._moments,
                    v_delta=self._v_delta, beta1=self.beta1, beta2=self.beta2, eps=self.eps_adam,
                    decay_1d=self.decay_1d, advance=bool(advance))

    def _update_adam(self, items, N, pp, hy, advance: bool, **r1):
        B = self.buf
        ext().psgd_update_adam(B.geom, B.ptrs, items, B.comm_buf, B.q_memory, float(N), B.q_warm,
                               2 if self.write_grad else 1, B.max_rank, geom_host=B._geom_host, p_prev=pp,
                               **self._adam_kw(advance, hy), **r1)

    def _rank1_adam(self, N, hy, advance: bool):
        r1 = slice(self.r1_start, self.arena_numel)
        ext().rank1_adam_step(self.buf.rank1_buf, float(N), self._m[r1], self.x[r1],
                              self.r1_upd if self.write_grad else None, **self._adam_kw(advance, hy))

    def adam_stats(self):
        """The AdamW block ``{"b1pow", "b2pow", "steps"}`` (a host sync on a device), or None with SGD."""
        return self.adam_state.read() if self.adam else None

    # -- helpers -------------------------------------------------------------------------
    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()
        self._reset_groups()

    def _reset_groups(self):
        for g in self.groups:
            g.ready = 0
            g.launched = False
        self._next_group = 0

    def _view(self, t, p):
        s = self.offsets[id(p)]
        return t[s: s + p.numel()]

    def _grads(self):
        gs = []
        for p in self.params:
            if p.grad is None:  # parameter unused this step: zero gradient
                p.grad = torch.zeros_like(p)
            g = p.grad
            assert g.is_contiguous() and g.dtype == torch.float32, "PowerSGD needs dense fp32 grads"
            gs.append(g)
        return gs

    def _bind(self):
        gmap = {id(p): p.grad for p in self.params}
        key = (upload_epoch(),) + tuple(g.data_ptr() for g in gmap.values())
        if key == self._grad_key:
            return
        B = self.buf
        rows, vec = [], []
        for p, (n, m) in zip(self.high, B.shapes):
            s = self.offsets[id(p)]
            g = gmap[id(p)].data_ptr()
            e, mo, x = (t[s:].data_ptr() for t in (self._e, self._m, self.x))
            row = [g, e, e, 0, 0, mo, x, g]
            rows.append(row)
            vec.append(B.vec_flag(len(vec), row))
        B.bind(rows, vec)
        pack, outs = [], []
        for p in self.rank1:
            s = self.offsets[id(p)] - self.r1_start
            pack.append((gmap[id(p)].view(-1), B.rank1_buf[s: s + p.numel()], 1, 0, 1.0))
            if self.write_grad:
                outs.append((self.r1_upd[s: s + p.numel()], gmap[id(p)].view(-1), 1, 0, 1.0))
        if B.fused:  # the P launch sums its split-K slabs itself and packs the rank-1 group
            self._r1_pack.set(pack)
        else:
            self._p_seg.set(B.p_seg_specs() + pack)
        self._r1_out.set(outs)
        self._grad_key = key

    def _init_queries(self):
        B = self.buf
        for i in range(len(B.shapes)):
            q = B.q_view(i)
            gen = torch.Generator(device=q.device)
            gen.manual_seed(int(self.rng.randint(1_000_000_000)))
            q.copy_(torch.randn(*q.shape, generator=gen, device=q.device, dtype=q.dtype))

    def _ensure_queries(self):
        """Draw the Q init once (reuse_query=True, reducer.py:101-111) or every step."""
        if self._q_ready:
            return
        assert not capturing(), \
            "run one eager step before capturing; reuse_query=False is not graph-capturable"
        self._init_queries()
        self._q_ready = True

    @property
    def bits_per_step(self) -> int:
        B = self.buf
        return 32 * (B.p_total + B.r1_numel + B.q_total)

    @property
    def collectives_per_step(self) -> int:
        if not self.comm.active:
            return 0
        if self.overlap:
            return 2 * len(self.groups) + (1 if self.r1_numel else 0)
        return 2 if self.buf.shapes else 1

    def collective_payloads(self) -> List[int]:
        """Bytes of every collective of one step, in issue order (link-model input)."""
        B = self.buf
        if self.overlap:
            out = []
            for g in self.groups:
                p0, p1 = B.p_range(g.lo, g.hi)
                q0, q1 = B.q_range(g.lo, g.hi)
                out += [4 * (p1 - p0), 4 * (q1 - q0)]
            if self.r1_numel:
                out.append(4 * self.r1_numel)
            return out
        return [4 * (B.p_total + self.r1_numel)] + ([4 * B.q_total] if B.shapes else [])

    def check_errors(self):
        """Host-synchronising health check (call at a low cadence: epoch / replica check):
        raises on a timed-out MGS barrier or an asynchronous RCCL error."""
        self.buf.check_orth()
        self.comm.check()

    @property
    def flat_weights(self) -> torch.Tensor:
        return self.x

    # attach_ema(): the EMA launch is the tail of phase_update (serial step and phases(), inside the
    # captured segment) or, with overlap groups, the last side-stream item, ahead of the release of
    # the next compute graph (the table may hold BatchNorm running statistics, which the next
    # forward rewrites)

    # -- the step --------------------------------------------------------------------------
    # Serial path: step() = phase_p -> comm_p -> phase_q -> comm_q -> phase_update.  The
    # phases are exposed separately so a piecewise hipGraph can capture the compute phases
    # and run the two collectives eagerly in between (utils/graph.py, c10d data plane).
    @torch.no_grad()
    def phase_p(self):
        B = self.buf
        self._ensure_queries()
        grads = self._grads()
        self._clip_grads(grads)  # before M = g + e: the error feedback sees the clipped gradient
        if not self.native:
            return
        self._sync_supports()
        self._bind()
        B.run_p(B.p_items, True, self.p_prev if self.lazy_ef else None,   # P (+ split-K sum + rank-1 pack)
                seg=self._r1_pack, p_seg=self._p_seg)

    @torch.no_grad()
    def comm_p(self):
        if self.native:
            self.comm.all_reduce(self.buf.comm_buf)            # [P | rank-1]: one collective

    @torch.no_grad()
    def phase_q(self):
        B = self.buf
        if self.native and B.shapes:
            B.orth(float(self.comm.world_size), self.eps, max_spins=self.orth_max_spins)
            B.run_q(B.q_items, B.q_seg)

    @torch.no_grad()
    def comm_q(self):
        if self.native and self.buf.shapes:
            self.comm.all_reduce(self.buf.q_memory)

    @torch.no_grad()
    def phase_update(self):
        B = self.buf
        N = self.comm.world_size
        if self.native:
            X = ext()
            r1 = slice(self.r1_start, self.arena_numel)
            hy = self._hyper_arg()
            if self.adam:
                pp = self.p_prev if self.lazy_ef else None
                ride = bool(B.shapes and B.fused and self.r1_numel)  # the rank-1 step rides in the update launch
                if ride:
                    self._update_adam(B.u_items, N, pp, hy, advance=True, r1_buf=B.rank1_buf, r1_div=float(N),
                                      r1_mom=self._m[r1], r1_x=self.x[r1],
                                      r1_g=self.r1_upd if self.write_grad else None)
                elif B.shapes:
                    self._update_adam(B.u_items, N, pp, hy, advance=not self.r1_numel)
                if self.r1_numel and not ride:
                    self._rank1_adam(N, hy, advance=True)
                if self.r1_numel and self.write_grad:
                    self._r1_out.run()
            elif B.shapes and B.fused and self.r1_numel:  # the rank-1 step rides in the update launch
                X.psgd_update(B.geom, B.ptrs, B.u_items, B.comm_buf, B.q_memory, float(N), B.q_warm,
                              2 if self.write_grad else 1, self.lr, self.momentum, B.max_rank,
                              self.p_prev if self.lazy_ef else None, r1_buf=B.rank1_buf, r1_div=float(N),
                              r1_mom=self._m[r1], r1_x=self.x[r1], r1_g=self.r1_upd if self.write_grad else None,
                              hyper=hy)
                if self.write_grad:
                    self._r1_out.run()
            elif B.shapes:
                X.psgd_update(B.geom, B.ptrs, B.u_items, B.comm_buf, B.q_memory, float(N), B.q_warm,
                              2 if self.write_grad else 1, self.lr, self.momentum, B.max_rank,
                              self.p_prev if self.lazy_ef else None, hyper=hy)
            if self.r1_numel and not (B.shapes and B.fused):
                X.rank1_step(B.rank1_buf, float(N), self._m[r1], self.x[r1],
                             self.r1_upd if self.write_grad else None, self.lr, self.momentum, hyper=hy)
                if self.write_grad:
                    self._r1_out.run()
        else:
            self._step_torch(N, [p.grad for p in self.params])
        self._after_update()
        self.count_step()

    def count_step(self):
        """Host-side bookkeeping of one step (graph replays call this explicitly)."""
        if capturing():  # the capture pass is not a real step
            return
        self._lazy_pending = self.lazy_ef
        self.step_count += 1
        self.bits_communicated += self.bits_per_step
        if not self.reuse_query:
            self._q_ready = False

    @torch.no_grad()
    def step(self) -> int:
        if self.overlap:
            self._finish_overlapped()
            self._reset_groups()
            self.count_step()
            return self.bits_per_step
        self.phase_p()
        self.comm_p()
        self.phase_q()
        self.comm_q()
        self.phase_update()
        return self.bits_per_step

    def phases(self):
        """[(fn, is_collective)] in execution order (for piecewise graph capture).  Piecewise
        capture runs the collectives eagerly between segments, so the hooks are disabled."""
        self.set_overlap(False)
        return [(self.phase_p, False), (self.comm_p, True), (self.phase_q, False), (self.comm_q, True),
                (self.phase_update, False)]

    def set_overlap(self, on: bool):
        if on and self.clip is not None:
            raise ValueError("PowerSGD: overlap=True cannot be combined with max_grad_norm > 0")
        if on and not self.groups:
            raise ValueError("optimizer was built without overlap groups")
        if self.hyper is not None and bool(on) != bool(self.overlap):
            # the block's uploads follow the update launches' stream (set_hyper): order both ways
            self.comm.fork()
            self.comm.join()
        self.overlap = on
        self._reset_groups()

    # -- hyper-parameter block -----------------------------------------------------------------
    # lr / weight_decay / hyper / _hyper_on, set_hyper() and plan_hyper(): ops/hyper.py HyperState
    def _hyper_on_side(self) -> bool:
        return bool(self.overlap)  # the update launches of the overlap groups run on the side stream

    def _check_hyper(self, lr: float, wd: float) -> None:
        """A captured step holds its dead-tap plan: switching the decay on or off under it raises.
        Under AdamW every matrix is always full: the plan does not depend on the decay."""
        if self.adam:
            return
        if self._captured_decay is not None and self._captured_decay != (wd != 0.0):
            raise RuntimeError("PowerSGD: weight_decay cannot be switched on or off after capture (the step "
                               "froze its dead-tap plan); capture again")
        if (wd != 0.0) != (self.weight_decay != 0.0):
            self._taps_seen = None  # decay on: every matrix full (_wanted_supports); off: compact again

    def _step_torch(self, N, grads):
        B = self.buf
        lam, lr, wd = self.momentum, self.lr, self.weight_decay
        gmap = {id(p): g for p, g in zip(self.params, grads)}
        Ms = []
        for i, p in enumerate(self.high):
            n, m = B.shapes[i]
            e = self._view(self._e, p)
            e.add_(gmap[id(p)].reshape(-1))              # M = g + e (stored in e)
            M = e.view(n, m)
            Ms.append(M)
            torch.matmul(M, B.q_view(i), out=B.p_view(i))
        for p in self.rank1:
            s = self.offsets[id(p)] - self.r1_start
            B.rank1_buf[s: s + p.numel()].copy_(gmap[id(p)].reshape(-1))
        self.comm.all_reduce(B.comm_buf)
        B.p_memory.div_(N)
        for i in range(len(self.high)):
            orthogonalize(B.p_view(i), self.eps)
        for i, M in enumerate(Ms):
            torch.matmul(M.t(), B.p_view(i), out=B.q_view(i, B.q_memory))
        self.comm.all_reduce(B.q_memory)
        B.q_memory.div_(N)
        B.q_warm.copy_(B.q_memory)
        if self.adam:  # the scalars of the block as it is before the step, for every tensor of it
            st = self.adam_state.read()
            S = adamw_scalars(st["b1pow"], st["b2pow"], lr, wd, self.beta1, self.beta2)
            decays_hi = np.float32(wd) != np.float32(0.0)
        for i, (p, M) in enumerate(zip(self.high, Ms)):
            out = torch.matmul(B.p_view(i), B.q_view(i).t()).view(-1)
            self._view(self._e, p).copy_(M.reshape(-1) - out)
            if self.adam:  # g := out, div = 1, every matrix decays
                _adamw_twin_(self._view(self.x, p), out, self._view(self._m, p), self._view(self._v, p), S,
                             self.beta1, self.beta2, self.eps_adam, 1.0, decays_hi)
                if self.write_grad:
                    gmap[id(p)].copy_(out.view_as(p))
                continue
            if wd != 0.0:  # after decompression and the error memory: d = out + wd x
                out = out.add(self._view(self.x, p), alpha=wd)
            mom = self._view(self._m, p)
            mom.mul_(lam).add_(out)
            upd = out + mom
            self._view(self.x, p).add_(upd, alpha=-lr)
            if self.write_grad:
                gmap[id(p)].copy_(upd.view_as(p))
        if self.adam:
            if self.r1_numel:  # g := rank1 / N (the twin divides, as the kernel does), decay_1d decides the decay
                r1 = slice(self.r1_start, self.arena_numel)
                _adamw_twin_(self.x[r1], B.rank1_buf, self._m[r1], self._v[r1], S, self.beta1, self.beta2,
                             self.eps_adam, float(N), bool(decays_hi) and self.decay_1d)
                if self.write_grad:
                    gg = B.rank1_buf if N == 1 else torch.div(B.rank1_buf, torch.tensor(float(N)))
                    for p in self.rank1:
                        s = self.offsets[id(p)] - self.r1_start
                        gmap[id(p)].copy_(gg[s: s + p.numel()].view_as(p))
            self.adam_state.write({"b1pow": float(S["p1"]), "b2pow": float(S["p2"]), "steps": st["steps"] + 1})
            return
        if self.r1_numel:
            r1 = slice(self.r1_start, self.arena_numel)
            out = B.rank1_buf / N
            if wd != 0.0:
                out = out.add(self.x[r1], alpha=wd)
            self._m[r1].mul_(lam).add_(out)
            upd = out + self._m[r1]
            self.x[r1].add_(upd, alpha=-lr)
            if self.write_grad:
                for p in self.rank1:
                    s = self.offsets[id(p)] - self.r1_start
                    gmap[id(p)].copy_(upd[s: s + p.numel()].view_as(p))

    # -- dead-tap compaction -----------------------------------------------------------------------
    def _wanted_supports(self) -> List[Tuple[int, int]]:
        """(T, mask) of every high-rank parameter whose recorded support has dead taps, else (0, 0).
        With weight decay a dead tap's weight still moves (d = wd x), so it needs its momentum:
        every matrix reports (0, 0), the full plan."""
        if self.weight_decay != 0.0 or self.adam:  # the AdamW update tile is the full one only
            return [(0, 0)] * len(self.high)
        out = []
        for p in self.high:
            s = taps.support_of(p) if p.dim() == 4 else None
            T = p.shape[2] * p.shape[3] if p.dim() == 4 else 0
            ok = (s is not None and s[0] == T and 2 <= T <= taps.MAX_PERIOD
                  and 0 < len(taps.tap_list(T, s[1])) < T)
            out.append((int(s[0]), int(s[1])) if ok else (0, 0))
        return out

    def _slot(self, arena: torch.Tensor, i: int, layout) -> torch.Tensor:
        """Matrix ``i``'s slot of an arena as [n, columns] in ``layout`` (None: full)."""
        n, m = self.buf.shapes[i]
        cols = m if layout is None else taps.compact_cols(m, *layout)
        s = self.offsets[id(self.high[i])]
        return arena[s: s + n * cols].view(n, cols)

    def _sync_supports(self):
        """Before a step's first reducer launch: re-plan if some conv's live-tap support changed."""
        if not self.dead_taps or self._taps_seen == taps.version():
            return
        seen = taps.version()
        want = self._wanted_supports()
        if [w if w[0] else None for w in want] != self.buf.layout:
            if capturing():
                raise RuntimeError("PowerSGD: a conv's live-tap support changed while capturing a graph; run one "
                                   "eager step on every input size first")
            self._replan(want)
        self._taps_seen = seen

    @torch.no_grad()
    def _replan(self, want: List[Tuple[int, int]]):
        """Convert the error-memory and momentum slots to the layout of ``want`` and rebuild the
        plan.  A matrix with a nonzero dead entry (a checkpoint trained at another resolution)
        stays full."""
        B = self.buf
        self.materialize_error()
        old = list(B.layout)
        want = list(want)
        for i, w in enumerate(want):
            if w[0] and old[i] != w:
                for arena in (self._e, self._m):
                    full = self._slot(arena, i, old[i])
                    if old[i] is not None:
                        full = taps.expand(full, B.shapes[i][1], *old[i])
                    if not taps.dead_all_zero(full, *w):
                        want[i] = (0, 0)
                        break
        new = [w if w[0] else None for w in want]
        for i in range(len(old)):  # compact -> full, in place
            if old[i] is not None and old[i] != new[i]:
                for arena in (self._e, self._m):
                    self._slot(arena, i, None).copy_(taps.expand(self._slot(arena, i, old[i]), B.shapes[i][1], *old[i]))
        B.replan(want)
        for i, lay in enumerate(B.layout):  # full -> compact (what the plan accepted), in place
            if lay is not None and lay != old[i]:
                for arena in (self._e, self._m):
                    full = self._slot(arena, i, None)
                    c = taps.compress(full, *lay).contiguous()
                    full.zero_()
                    self._slot(arena, i, lay).copy_(c)
        self._grad_key = None
        for g in self.groups:
            g.key = None

    def _full_arena(self, arena: torch.Tensor) -> torch.Tensor:
        """``arena`` in the full reference layout (the arena itself when nothing is compacted)."""
        B = self.buf
        if all(lay is None for lay in B.layout):
            return arena
        out = arena.clone()
        for i, lay in enumerate(B.layout):
            if lay is not None:
                s = self.offsets[id(self.high[i])]
                n, m = B.shapes[i]
                out[s: s + n * m].view(n, m).copy_(taps.expand(self._slot(arena, i, lay), m, *lay))
        return out

    def _load_arena(self, arena: torch.Tensor, full: torch.Tensor):
        """Copy a full-layout arena image into ``arena`` in the plan's layout."""
        B = self.buf
        arena.copy_(full)
        for i, lay in enumerate(B.layout):
            if lay is not None:
                slot = self._slot(arena, i, None)
                c = taps.compress(slot, *lay).contiguous()
                slot.zero_()
                self._slot(arena, i, lay).copy_(c)

    @property
    def m(self) -> torch.Tensor:
        """The momentum arena in the full reference layout (a copy when a matrix is compacted)."""
        return self._full_arena(self._m)

    # -- lazy error feedback -------------------------------------------------------------------
    @property
    def e(self) -> torch.Tensor:
        """The error-feedback memory (reducer.py ``memories``), materialised: with lazy error
        feedback the arena holds ``M`` and the correction ``- P_prev Qs^T`` is applied here by
        the update kernel's own arithmetic (mode 3), exactly as the next P pass would.  Full
        reference layout (a copy when a matrix is dead-tap compacted)."""
        self.materialize_error()
        return self._full_arena(self._e)

    @torch.no_grad()
    def materialize_error(self):
        if not (self.lazy_ef and self._lazy_pending) or capturing():
            return
        B = self.buf
        ext().psgd_update(B.geom, B.ptrs, B.u_items, self.p_prev, B.q_warm, 1.0, None, 3, 0.0, 0.0, B.max_rank)
        self.p_prev.zero_()
        self._lazy_pending = False

    # -- training-state snapshot (graph warm-up must not change training) -------------------
    def prepare(self):
        """Draw the initial queries now (before a graph warm-up snapshot)."""
        with torch.no_grad():
            self._ensure_queries()

    def snapshot(self):
        # e / m in the full layout: the warm-up steps between snapshot and restore may re-plan
        return {**self._snapshot_extras(),
                "x": self.x.clone(), "e": self._full_arena(self._e).clone(), "p_prev": self.p_prev.clone(),
                "lazy_pending": self._lazy_pending, "m": self.m.clone(), "q": self.buf.q_warm.clone(),
                "step_count": self.step_count, "bits": self.bits_communicated, "q_ready": self._q_ready,
                "rng": self.rng.get_state(),
                **({"v": self._v.clone(), "adam": self.adam_state.snapshot()} if self.adam else {})}

    def restore(self, snap):
        self.x.copy_(snap["x"])
        self._load_arena(self._e, snap["e"])
        self.p_prev.copy_(snap["p_prev"])
        self._lazy_pending = snap["lazy_pending"]
        self._load_arena(self._m, snap["m"])
        self.buf.q_warm.copy_(snap["q"])
        self.step_count = snap["step_count"]
        self.bits_communicated = snap["bits"]
        self._q_ready = snap["q_ready"]
        self.rng.set_state(snap["rng"])
        if self.adam:
            self._v.copy_(snap["v"])
            self.adam_state.restore(snap["adam"])
        self._restore_extras(snap)

    # -- checkpoint / resume ---------------------------------------------------------------
    def state_dict(self):
        adam = {}
        if self.adam:  # "momentum" is the first moment
            st = self.adam_state.read()
            adam = {"optimizer": "adamw", "exp_avg_sq": self._v.detach().cpu().clone(), "b1pow": st["b1pow"],
                    "b2pow": st["b2pow"], "steps": st["steps"], "betas": (self.beta1, self.beta2),
                    "eps_adam": self.eps_adam, "decay_1d": self.decay_1d}
        return {
            **adam,
            "step_count": self.step_count,
            "bits_communicated": self.bits_communicated,
            "error": self.e.detach().cpu().clone(),  # materialised (lazy error feedback)
            "momentum": self.m.detach().cpu().clone(),
            "q_warm": self.buf.q_warm.detach().cpu().clone(),
            "q_ready": self._q_ready,
            "rng_state": _rng_state_to_dict(self.rng.get_state()),
            "lr": self.lr,
            "weight_decay": self.weight_decay,
            "momentum_coef": self.momentum,
            "rank": self.rank,
        }

    def load_state_dict(self, sd):
        assert sd["rank"] == self.rank, "checkpoint compression rank differs"
        theirs = sd.get("optimizer", "sgd")  # a checkpoint without "optimizer" is an SGD checkpoint
        if theirs != self.optimizer:
            raise ValueError(f"PowerSGD: the checkpoint holds {theirs} optimizer state, this sync runs "
                             f"{self.optimizer}; they cannot be loaded into each other")
        self.step_count = int(sd["step_count"])
        self.bits_communicated = int(sd["bits_communicated"])
        if any(lay is not None for lay in self.buf.layout):
            # back to the full layout; the next step compacts again what the loaded state allows
            self._replan([(0, 0)] * len(self.high))
        self._taps_seen = None
        self._e.copy_(sd["error"])
        self.p_prev.zero_()  # e is the true error memory: no pending correction
        self._lazy_pending = False
        self._m.copy_(sd["momentum"])
        if self.adam:
            self._v.copy_(sd["exp_avg_sq"])
            self.adam_state.write({"b1pow": float(np.float32(sd["b1pow"])), "b2pow": float(np.float32(sd["b2pow"])),
                                   "steps": int(sd["steps"])})
        self.buf.q_warm.copy_(sd["q_warm"])
        self._q_ready = bool(sd.get("q_ready", self.step_count > 0)) and self.reuse_query
        self.rng.set_state(_rng_state_from_dict(sd["rng_state"]))
        self.momentum = float(sd["momentum_coef"])
        self._load_hyper(float(sd["lr"]), float(sd.get("weight_decay", 0.0)))


def _rng_state_to_dict(st):
    name, keys, pos, has_gauss, cached = st
    return {"name": name, "keys": torch.from_numpy(np.asarray(keys, dtype=np.int64)), "pos": int(pos),
            "has_gauss": int(has_gauss), "cached": float(cached)}


def _rng_state_from_dict(d):
    return (d["name"], d["keys"].numpy().astype(np.uint32), d["pos"], d["has_gauss"], d["cached"])
