"""The weight-EMA rule, test-only: numpy float32, one operation per line, no framework import.

``n`` earlier runs, ``decay`` in (0, 1), ``warmup``:
    d = min(decay, (n + 1) / (n + 10))  with warm-up, else decay;   w = 1 - d
    every element:  t = x - s;  u = w * t;  s' = s + u
Every line is one correctly rounded fp32 operation (numpy float32 arithmetic rounds each result
to nearest-even, division included).  ``fused`` is the rule a contracted kernel would compute
instead: w * t + s in fp64, rounded to fp32 once; the tests require inputs on which it differs.
"""
import numpy as np

F = np.float32


def rule_decay(decay, n, warmup):
    """(d, w) of the run that follows ``n`` earlier ones."""
    d = F(decay)
    if warmup:
        fn = F(np.uint32(n))       # (float)n, round to nearest
        num = fn + F(1.0)
        den = fn + F(10.0)
        r = num / den
        d = r if r < d else d
    w = F(1.0) - d
    return F(d), F(w)


def rule_update(x, s, w):
    """The shadow after one run with weight ``w``; x, s float32 arrays of one shape."""
    x = np.asarray(x, dtype=F)
    s = np.asarray(s, dtype=F)
    with np.errstate(all="ignore"):
        t = x - s
        u = F(w) * t
        out = s + u
    assert t.dtype == F and u.dtype == F and out.dtype == F
    return out


def rule_run(xs, s0, decay, warmup, n0=0):
    """Shadows and blocks after each of the runs whose live values are ``xs`` (a list of arrays)."""
    s = np.array(s0, dtype=F, copy=True)
    out = []
    for k, x in enumerate(xs):
        d, w = rule_decay(decay, n0 + k, warmup)
        s = rule_update(x, s, w)
        out.append((s.copy(), (d, w, n0 + k + 1)))
    return out


def fused_update(x, s, w):
    """fma(w, x - s, s): the product unrounded (fp64 holds it exactly), one rounding at the end."""
    x = np.asarray(x, dtype=F)
    s = np.asarray(s, dtype=F)
    with np.errstate(all="ignore"):
        t = x - s
        return (np.float64(F(w)) * t.astype(np.float64) + s.astype(np.float64)).astype(F)


def gaussians(seed, n):
    """``n`` seeded normal-range fp32 Gaussians with full mantissas (no denormals, no zeros)."""
    g = np.random.default_rng(seed).standard_normal(n).astype(F)
    tiny = np.abs(g) < F(2.0 ** -100)
    g[tiny] = F(1.0)
    return g


def special_pairs():
    """(x, s) holding +-0, +-inf, NaN and x == s."""
    inf, nan = F(np.inf), F(np.nan)
    x = np.array([0.0, -0.0, 0.0, -0.0, inf, -inf, inf, 1.0, nan, 1.0, 2.5, -3.0, 1e-3, 7.0], dtype=F)
    s = np.array([0.0, -0.0, -0.0, 0.0, inf, -inf, -inf, inf, 1.0, nan, 2.5, -3.0, 1e-3, -7.0], dtype=F)
    return x, s


def same_bits(a, b):
    """Bitwise equality, NaN compared by position (payloads ignored)."""
    a = np.asarray(a, dtype=F)
    b = np.asarray(b, dtype=F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    return np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])
