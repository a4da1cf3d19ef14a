"""Independent rules for the DistilBERT kernels (csrc/attention.hip, layernorm.hip, linear.hip,
embedding.hip): pure torch, no extension, nothing imported from ops/.

  * the two keep-mask hashes, written out from the kernels' text (attn_hash = hash4 of
    csrc/attention.hip, ln_hash of csrc/layernorm.hip) with 32-bit products split into 16-bit halves, so
    that no intermediate leaves int64; an element is kept iff hash >= thr64(p);
  * thr64(p), the dropout threshold in double (bindings.cpp ln_drop), and thr32(p), the threshold the
    attention launchers used to compute in fp32: hashes in [thr64, thr32) are the elements on which the
    two disagree (tests/bert_kernel_cases.py names some);
  * twins of the launch geometry: colsum_chunks / rows_per_chunk (csrc/linear.hip), ln_bwd_wgs /
    rows_per_wave (csrc/layernorm.hip);
  * fp64 rules: attention (HF masked softmax with finfo(float32).min), add + LayerNorm with both
    dropout placements, PyTorch's exact GELU backward, column sums, embedding backward;
  * exact fp32 order emulations of the sums that are pure additions (nothing an FMA could contract):
    the column sums, LayerNorm's dbeta without output dropout, the embedding row sums, and the slab
    sum (conv_slab_sum_kernel) that finishes the first two.
"""
from __future__ import annotations

import math

import torch

M32 = 0xFFFFFFFF
F32_MIN = torch.finfo(torch.float32).min


# ------------------------------------------------ hashes ------------------------------------------------
def _mul32(x, c: int):
    """(x * c) mod 2^32 for x in [0, 2^32) (int or int64 tensor) without leaving 48 bits"""
    lo = x * (c & 0xFFFF)
    hi = (x * (c >> 16)) & 0xFFFF
    return (lo + (hi << 16)) & M32


def _i64(x):
    return x.to(torch.int64) if isinstance(x, torch.Tensor) else int(x)


def attn_hash(seed: int, bh, q, k):
    """hash4(seed, bh, q, k) of csrc/attention.hip; bh / q / k: ints or broadcastable int64 tensors"""
    a, b, c, d = int(seed) & M32, _i64(bh), _i64(q), _i64(k)
    h = _mul32(a, 0x9E3779B1) ^ _mul32((b + 0x7F4A7C15) & M32, 0x85EBCA77)
    h = h ^ _mul32((c + 0x165667B1) & M32, 0xC2B2AE3D)
    h = _mul32(h ^ (h >> 15), 0x2C1B3C6D)
    h = h ^ _mul32((d + 0x27D4EB2F) & M32, 0x9E3779B1)
    h = _mul32(h ^ (h >> 13), 0x297A2D39)
    return h ^ (h >> 16)


def ln_hash(seed: int, row, col):
    """ln_hash(seed, row, col) of csrc/layernorm.hip"""
    a, r, c = int(seed) & M32, _i64(row), _i64(col)
    h = _mul32(a, 0x9E3779B1) ^ _mul32((r + 0x7F4A7C15) & M32, 0x85EBCA77)
    h = _mul32(h ^ (h >> 15), 0x2C1B3C6D)
    h = h ^ _mul32((c + 0x165667B1) & M32, 0xC2B2AE3D)
    h = _mul32(h ^ (h >> 13), 0x297A2D39)
    return h ^ (h >> 16)


def thr64(p: float) -> int:
    """the dropout threshold, in double"""
    return min(int(p * 2 ** 32), M32)


def thr32(p: float) -> int:
    """the threshold as fp32 arithmetic gives it: float(p) * 2^32 (exact: a power of two), capped"""
    pf = torch.tensor(p, dtype=torch.float32).item()  # p rounded to fp32, held exactly in a double
    return min(int(pf * 2 ** 32), M32)


def attn_keep(seed: int, BH: int, S: int, p: float, device="cpu") -> torch.Tensor:
    """[BH, S(query), S(key)] bool"""
    ar = lambda n, shape: torch.arange(n, dtype=torch.int64, device=device).view(shape)  # noqa: E731
    return attn_hash(seed, ar(BH, (-1, 1, 1)), ar(S, (1, -1, 1)), ar(S, (1, 1, -1))) >= thr64(p)


def ln_keep(seed: int, R: int, D: int, p: float, device="cpu") -> torch.Tensor:
    """[R, D] bool"""
    r = torch.arange(R, dtype=torch.int64, device=device).view(-1, 1)
    c = torch.arange(D, dtype=torch.int64, device=device).view(1, -1)
    return ln_hash(seed, r, c) >= thr64(p)


# ------------------------------------------- launch geometry --------------------------------------------
def colsum_strips(N: int) -> int:
    return (N // 4 + 63) // 64


def colsum_chunks(M: int, N: int) -> int:
    chunks = (1024 + colsum_strips(N) - 1) // colsum_strips(N)
    chunks = min(chunks, (M + 31) // 32)
    return max(chunks, 1)


def rows_per_chunk(M: int, N: int) -> int:
    c = colsum_chunks(M, N)
    return (M + c - 1) // c


def group_rows(M: int, N: int):
    """rows each of the 4 lane groups adds, per chunk: a list (one entry per chunk) of 4 counts"""
    rpc = rows_per_chunk(M, N)
    out = []
    for c in range(colsum_chunks(M, N)):
        r0, r1 = c * rpc, min(M, (c + 1) * rpc)
        out.append([len(range(r0 + g, r1, 4)) for g in range(4)])
    return out


def ln_bwd_wgs(R: int) -> int:
    return max(1, min(512, (R + 3) // 4))


def rows_per_wave(R: int) -> int:
    w = ln_bwd_wgs(R)
    return (R + 4 * w - 1) // (4 * w)


# ---------------------------------------------- fp64 rules ----------------------------------------------
def attention_rule(q, k, v, mask=None, keep=None, p: float = 0.0, dout=None):
    """q / k / v / dout [B, S, H, D] (any float dtype; computed in fp64), mask [B, S] (nonzero = attend) or
    None, keep [B * H, S, S] bool or None.  Returns o, dq, dk, dv [B, S, H, D], m, logl, delta [B, H, S]:
    m the row maximum of the masked scaled scores, logl = log(sum exp(score - m)) before dropout."""
    B, S, H, D = q.shape
    qt, kt, vt = (t.double().transpose(1, 2) for t in (q, k, v))  # [B, H, S, D]
    scale = 1.0 / math.sqrt(D)
    s = torch.matmul(qt * scale, kt.transpose(-1, -2))
    dead = None
    if mask is not None:
        dead = (mask == 0).view(B, 1, 1, S)
        s = s.masked_fill(dead, F32_MIN)
    m = s.amax(-1)
    s.sub_(m.unsqueeze(-1)).exp_()
    l = s.sum(-1)
    P = s.div_(l.unsqueeze(-1))
    kf = None
    if keep is not None:
        kf = keep.view(B, H, S, S).double() / (1.0 - p)
    Pd = P * kf if kf is not None else P
    out = {"o": torch.matmul(Pd, vt).transpose(1, 2).contiguous(), "m": m, "logl": l.log()}
    if dout is None:
        return out
    g = dout.double().transpose(1, 2)
    out["dv"] = torch.matmul(Pd.transpose(-1, -2), g).transpose(1, 2).contiguous()
    del Pd
    dP = torch.matmul(g, vt.transpose(-1, -2))
    if kf is not None:
        dP.mul_(kf)
    delta = (g * out["o"].transpose(1, 2)).sum(-1)
    dS = dP.sub_(delta.unsqueeze(-1)).mul_(P)
    if dead is not None:
        dS.masked_fill_(dead, 0.0)  # masked_fill passes no gradient to the score
    out["dq"] = (torch.matmul(dS, kt) * scale).transpose(1, 2).contiguous()
    out["dk"] = (torch.matmul(dS.transpose(-1, -2), qt) * scale).transpose(1, 2).contiguous()
    out["delta"] = delta
    return out


def add_ln_rule(a, b, gamma, beta, eps: float, mode: int = 0, keep=None, p: float = 0.0, dy=None):
    """y = LN(drop(a) + b) (mode 1), drop(LN(a + b)) (mode 2), LN(a + b) (mode 0); a / b / dy [R, D], b may
    be None.  Returns y, s, mean, rstd and, with dy, dx (the gradient of s, i.e. of b), da, dgamma, dbeta."""
    a, gamma, beta = a.double(), gamma.double(), beta.double()
    kf = keep.double() / (1.0 - p) if mode else None
    s = a * kf if mode == 1 else a.clone()
    if b is not None:
        s = s + b.double()
    mean = s.mean(-1, keepdim=True)
    var = ((s - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (s - mean) * rstd
    y = xh * gamma + beta
    if mode == 2:
        y = y * kf
    out = {"y": y, "s": s, "mean": mean.squeeze(-1), "rstd": rstd.squeeze(-1)}
    if dy is None:
        return out
    d = dy.double() * kf if mode == 2 else dy.double()
    g = d * gamma
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    out.update(dx=dx, da=dx * kf if mode == 1 else dx, dgamma=(d * xh).sum(0), dbeta=d.sum(0))
    return out


def gelu_bwd_rule(g, h):
    """PyTorch's exact (approximate='none') GELU backward, fp64"""
    g, h = g.double(), h.double()
    cdf = 0.5 * (1.0 + torch.erf(h * math.sqrt(0.5)))
    pdf = torch.exp(-0.5 * h * h) * (1.0 / math.sqrt(2.0 * math.pi))
    return g * (cdf + h * pdf)


def colsum_rule(g):
    return g.double().sum(0)


def emb_valid(ids, V: int, pad):
    """tokens that contribute: id in [0, V) and not the padding id"""
    ok = (ids >= 0) & (ids < V)
    return ok & (ids != pad) if pad is not None else ok


def embedding_bwd_rule(ids, gout, V: int, pad):
    """fp64 grad_W [V, D]"""
    ids = ids.reshape(-1)
    ok = emb_valid(ids, V, pad)
    gw = torch.zeros(V, gout.shape[-1], dtype=torch.float64, device=gout.device)
    return gw.index_add_(0, ids[ok], gout.reshape(-1, gout.shape[-1]).double()[ok])


# ------------------------------------------ fp32 order emulations ---------------------------------------
def slab_sum_order(part, n: int, numel: int):
    """The fp32 sum of n slabs of numel floats in the order of conv_slab_sum_kernel: group g adds slabs g,
    g + 16, ... onto zero, then the 16 groups are added in order (as _slab_sum of
    tests/test_conv_plans_gpu.py)."""
    assert part.dtype == torch.float32
    s = part.reshape(-1)[: n * numel].view(n, numel)
    acc = torch.zeros(min(n, 16), numel, device=part.device)
    for j in range(0, n, 16):
        c = s[j: j + 16]
        acc[: c.shape[0]] += c
    t = acc[0].clone()
    for k in range(1, acc.shape[0]):
        t += acc[k]
    return t


def _strided_row_sums(x, starts, ends, stride: int):
    """acc[i] = ((0 + x[starts[i]]) + x[starts[i] + stride]) + ... over rows < ends[i], fp32, in order"""
    assert x.dtype == torch.float32
    acc = torch.zeros(len(starts), x.shape[1], device=x.device)
    st = torch.tensor(starts, dtype=torch.int64, device=x.device)
    en = torch.tensor(ends, dtype=torch.int64, device=x.device)
    steps = max([len(range(s, e, stride)) for s, e in zip(starts, ends)] + [0])
    for j in range(steps):
        r = st + j * stride
        live = r < en
        acc[live] = acc[live] + x[r[live]]
    return acc


def colsum_partials_order(g):
    """part [chunks, N] of colsum_partial_kernel: per chunk, lane group k adds rows r0 + k, r0 + k + 4, ...
    in order (the unrolled loop and its tail add in the same order), then ((g0 + g1) + g2) + g3"""
    M, N = g.shape
    chunks, rpc = colsum_chunks(M, N), rows_per_chunk(M, N)
    starts = [c * rpc + k for c in range(chunks) for k in range(4)]
    ends = [min(M, (c + 1) * rpc) for c in range(chunks) for _ in range(4)]
    a = _strided_row_sums(g, starts, ends, 4).view(chunks, 4, N)
    return ((a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3]


def colsum_order(g):
    part = colsum_partials_order(g)
    return slab_sum_order(part, part.shape[0], g.shape[1])


def ln_dbeta_partials_order(d):
    """the dbeta half of ln_bwd_kernel's per-workgroup partials, [wgs, D], for d = dy [R, D] (dropout
    modes 0 and 1): wave w of workgroup b adds rows (4 b + w) rpw + k, k < rpw, in order, then the 4 waves
    are added in order"""
    R, D = d.shape
    wgs, rpw = ln_bwd_wgs(R), rows_per_wave(R)
    starts = [(4 * b + w) * rpw for b in range(wgs) for w in range(4)]
    ends = [min(R, s + rpw) for s in starts]
    a = _strided_row_sums(d, starts, ends, 1).view(wgs, 4, D)
    return ((a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3]


def ln_dbeta_order(d):
    part = ln_dbeta_partials_order(d)
    return slab_sum_order(part, part.shape[0], d.shape[1])


def embedding_bwd_order(ids, gout, V: int, pad):
    """fp32 grad_W [V, D]: each row the sum of its tokens' gradient rows in increasing token order, onto
    zero (computed on the CPU; returned on gout's device)"""
    ids_c = ids.reshape(-1).cpu()
    g = gout.reshape(-1, gout.shape[-1]).float().cpu()
    ok = emb_valid(ids_c, V, pad)
    gw = torch.zeros(V, g.shape[1])
    # occurrence j of every id at once: tokens of one id keep their order, ids do not interact
    toks = torch.nonzero(ok).view(-1)
    if toks.numel():
        v = ids_c[toks]
        order = torch.argsort(v, stable=True)
        toks, v = toks[order], v[order]
        first = torch.ones_like(v, dtype=torch.bool)
        first[1:] = v[1:] != v[:-1]
        start = torch.nonzero(first).view(-1)
        rank = torch.arange(v.numel()) - start[torch.cumsum(first.long(), 0) - 1]
        for j in range(int(rank.max()) + 1):
            sel = rank == j
            gw[v[sel]] = gw[v[sel]] + g[toks[sel]]
    return gw.to(gout.device)
