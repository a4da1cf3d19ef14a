"""The AdamW rule, test-only: loops over numpy float32 scalars, one operation per line, no framework
import; written independently of the torch twin in ops/adamw.py.

Block ``(b1pow, b2pow, steps)`` starts as ``(1, 1, 0)``.  Per launch:
    p1 = b1pow * beta1;  p2 = b2pow * beta2;  bc1 = 1 - p1;  bc2 = 1 - p2;  ss = lr / bc1;
    sb = sqrt(bc2);  om1 = 1 - beta1;  om2 = 1 - beta2;  c = 1 - lr * wd
per element:
    gg = g / div (div != 1);  x1 = x * c (wd != 0 and the entry decays);
    m' = (beta1 * m) + (om1 * gg);  v' = (beta2 * v) + (om2 * (gg * gg));
    den = (sqrt(v') / sb) + eps;  x' = x1 - ss * (m' / den)
and the block becomes ``(p1, p2, steps + 1)``.  Every line is one correctly rounded fp32 operation
(numpy float32 scalar arithmetic rounds each result to nearest-even; division and sqrt included).

``contracted`` names the rule a contracting compiler would compute instead, with one product left
unrounded (fp64 holds a product of two fp32 values exactly) and one rounding at the end:
``"m"``: fma(beta1, m, om1 * gg);  ``"v"``: fma(beta2, v, om2 * (gg * gg));
``"x"``: fma(-ss, m' / den, x1).  The tests require inputs on which each differs from the rule.
"""
import numpy as np

F = np.float32
D = np.float64
CONTRACTED = ("m", "v", "x")


def scalars(block, lr, wd, beta1, beta2):
    """The per-launch scalars from the block before the launch."""
    b1pow, b2pow, _ = block
    with np.errstate(all="ignore"):
        p1 = F(b1pow) * F(beta1)
        p2 = F(b2pow) * F(beta2)
        bc1 = F(1.0) - p1
        bc2 = F(1.0) - p2
        ss = F(lr) / bc1
        sb = F(np.sqrt(bc2))
        om1 = F(1.0) - F(beta1)
        om2 = F(1.0) - F(beta2)
        lw = F(lr) * F(wd)
        c = F(1.0) - lw
    for s in (p1, p2, bc1, bc2, ss, sb, om1, om2, c):
        assert type(s) is F
    return dict(p1=p1, p2=p2, bc1=bc1, bc2=bc2, ss=ss, sb=sb, om1=om1, om2=om2, c=c)


def element(x, g, m, v, S, beta1, beta2, eps, div, decays, wd, contracted=None):
    """(x', m', v') of one element, every argument a numpy float32 scalar (``step`` loops over
    them); float32 arrays of one shape go through the same lines, each still one rounded operation
    per element (``step_arrays``, for inputs too large to loop over)."""
    with np.errstate(all="ignore"):
        gg = g / F(div) if F(div) != F(1.0) else g
        x1 = x * S["c"] if (F(wd) != F(0.0) and decays) else x
        a = F(beta1) * m
        b = S["om1"] * gg
        if contracted == "m":
            mn = _f(D(F(beta1)) * _d(m) + _d(b))
        else:
            mn = a + b
        g2 = gg * gg
        d = F(beta2) * v
        e = S["om2"] * g2
        if contracted == "v":
            vn = _f(D(F(beta2)) * _d(v) + _d(e))
        else:
            vn = d + e
        r = np.sqrt(vn)
        t = r / S["sb"]
        den = t + F(eps)
        q = mn / den
        if contracted == "x":
            xn = _f(_d(x1) - D(S["ss"]) * _d(q))
        else:
            u = S["ss"] * q
            xn = x1 - u
    assert all(np.asarray(t).dtype == F for t in (gg, x1, a, b, g2, d, e, r, t, den, q, xn, mn, vn))
    return xn, mn, vn


def _d(a):
    return np.asarray(a, dtype=F).astype(D)[()]


def _f(a):
    return np.asarray(a, dtype=D).astype(F)[()]


def step_arrays(x, g, m, v, block, lr, wd, beta1, beta2, eps, div=1.0, decays=True, contracted=None):
    """``step`` with the element lines applied to whole arrays."""
    x, g, m, v = (np.asarray(t, dtype=F).ravel() for t in (x, g, m, v))
    S = scalars(block, lr, wd, beta1, beta2)
    xo, mo, vo = element(x, g, m, v, S, beta1, beta2, eps, div, decays, wd, contracted)
    return xo, mo, vo, (S["p1"], S["p2"], int(block[2]) + 1)


def step(x, g, m, v, block, lr, wd, beta1, beta2, eps, div=1.0, decays=True, contracted=None):
    """One launch over float32 arrays of one shape: (x', m', v', block')."""
    x, g, m, v = (np.asarray(t, dtype=F).ravel() for t in (x, g, m, v))
    S = scalars(block, lr, wd, beta1, beta2)
    xo, mo, vo = np.empty_like(x), np.empty_like(m), np.empty_like(v)
    for i in range(x.size):
        xo[i], mo[i], vo[i] = element(x[i], g[i], m[i], v[i], S, beta1, beta2, eps, div, decays, wd, contracted)
    return xo, mo, vo, (S["p1"], S["p2"], int(block[2]) + 1)


def run(x0, gs, lr, wd, beta1, beta2, eps, div=1.0, decays=True, contracted=None):
    """The states after each of the launches whose gradients are ``gs``, from zero moments and the
    initial block: a list of (x, m, v, block)."""
    x = np.array(x0, dtype=F, copy=True).ravel()
    m, v = np.zeros_like(x), np.zeros_like(x)
    block = (F(1.0), F(1.0), 0)
    out = []
    for g in gs:
        x, m, v, block = step(x, g, m, v, block, lr, wd, beta1, beta2, eps, div, decays, contracted)
        out.append((x.copy(), m.copy(), v.copy(), block))
    return out


def gaussians(seed, n, scale=1.0):
    """``n`` seeded normal-range fp32 Gaussians with full mantissas (no denormals, no zeros)."""
    g = (np.random.default_rng(seed).standard_normal(n) * scale).astype(F)
    g[np.abs(g) < F(2.0 ** -100)] = F(1.0)
    return g


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
