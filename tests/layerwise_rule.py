"""The LAMB / LARS rules of ops/layerwise.py, test-only: a plain numpy reference per tensor, the table
of shapes, and the one check that the CPU (twin) and GPU (kernel) tests share.

What the reference takes as given, and why.  The rules define ``m'``, ``v'``, ``u`` and ``gg`` as fp32
values (one rounded operation per line) and the norms as fp64 sums OVER those fp32 values, so the
reference forms them exactly so: ``m'``, ``v'`` by tests/adamw_rule.py (checked bitwise), ``u`` by the
same kind of one-operation-per-line numpy float32 arithmetic, with the launch scalars of
``adamw_rule.scalars``.  From there everything is fp64: the sums, ``trust_t`` (left unrounded),
and ``x'`` from the fp32 ``m'``, ``v'``, ``x`` (and ``b'`` from the fp32 ``gg``, ``b``, ``x``).

Bounds (u = 2^-24, the unit roundoff).  ``trust_t``: 2 fp32 ulps (one rounding, one for the summation
order).  LAMB ``x'``: sqrt, / sb, + eps, m' / den, / bc1, wd x and the add reach ``u`` in at most 8
roundings: 8u (|r| + wd |x|) = 2^-21 (...); with the trust error, the two products and the
subtraction, doubled: ``2^-24 |x'| + 2^-19 lr trust (|r| + wd |x|)``.  LARS: the decay fma, ``lam_t``, the
product and the momentum fma: 4u = ``2^-22 (mu |b| + lam (|gg| + wd |x|))`` on ``b'``, and with the last fma
``2^-24 |x'| + 2^-21 lr (mu |b| + lam (|gg| + wd |x|))`` on ``x'``.
"""
import numpy as np
import torch

from network_distributed_pytorch_amd import ops

from . import adamw_rule as R

F, D = np.float32, np.float64
LR, B1, B2, EPS, MU, ETA, EPS_L = 1e-2, 0.9, 0.999, 1e-8, 0.9, 0.001, 1e-8
# name -> (numel, elements past a 16-byte boundary, adapts, x == 0, g == 0)
TENSORS = {"one": (1, 0, True, False, False), "n2047": (2047, 0, True, False, False),
           "n2048": (2048, 0, True, False, False), "n2049": (2049, 0, True, False, False),
           "scalar_path": (4099, 1, True, False, False), "x_zero": (300, 0, True, True, False),
           "g_zero": (300, 0, True, False, True), "exempt_1d": (513, 0, False, False, False),
           "blocks70": (70 * 2048, 0, True, False, False)}  # > 64 blocks: a second first-level ticket group


def ulps(got, ref) -> float:
    return abs(float(got) - float(ref)) / float(np.spacing(F(abs(ref))))


def ref_lamb(x, g, m, v, block, lr, wd, div, adapts):
    """One tensor, one step: ``(m', v', trust, x', bound on x')``."""
    dec = adapts and F(wd) != 0
    S = R.scalars(block, lr, wd, B1, B2)
    _, mo, vo, _ = R.step_arrays(x, g, m, v, block, lr, wd, B1, B2, EPS, div)
    with np.errstate(all="ignore"):
        r32 = ((mo / ((np.sqrt(vo) / S["sb"]) + F(EPS))) / S["bc1"])
        u32 = r32 + F(wd) * x if dec else r32
        W, U = np.sqrt(np.sum(x.astype(D) ** 2)), np.sqrt(np.sum(u32.astype(D) ** 2))
        trust = W / U if adapts and W > 0 and U > 0 else 1.0
        r = (mo.astype(D) / (np.sqrt(vo.astype(D)) / D(S["sb"]) + D(F(EPS)))) / D(S["bc1"])
        w, xd = D(F(wd)) if dec else 0.0, x.astype(D)
        xn = xd - D(F(lr)) * trust * (r + w * xd)
    return mo, vo, trust, xn, 2.0 ** -24 * np.abs(xn) + 2.0 ** -19 * D(F(lr)) * trust * (np.abs(r) + w * np.abs(xd))


def ref_lars(x, g, b, lr, wd, div, adapts):
    """One tensor, one step: ``(b', bound on b', lam, x', bound on x')``."""
    with np.errstate(all="ignore"):
        gg, x, b = (g / F(div) if F(div) != 1 else g).astype(D), x.astype(D), b.astype(D)
        W, G = np.sqrt(np.sum(x ** 2)), np.sqrt(np.sum(gg ** 2))
        lam = D(F(ETA)) * W / (G + D(F(wd)) * W + D(F(EPS_L))) if adapts and W > 0 and G > 0 else 1.0
        w = D(F(wd)) if adapts else 0.0
        bn = D(F(MU)) * b + lam * (gg + w * x)
        mag = D(F(MU)) * np.abs(b) + lam * (np.abs(gg) + w * np.abs(x))
        xn = x - D(F(lr)) * bn
    return bn, 2.0 ** -22 * mag, lam, xn, 2.0 ** -24 * np.abs(xn) + 2.0 ** -21 * D(F(lr)) * mag


def check_tensor(kind, name, pre, post, trust, block, lr, wd, div, adapts):
    """``pre`` = (x, g, m, v | x, g, b), ``post`` = (x', m', v' | x', b') as float32 arrays of one tensor."""
    if kind == "lamb":
        mo, vo, tref, xref, bound = ref_lamb(*pre, block, lr, wd, div, adapts)
        assert R.same_bits(post[1], mo) and R.same_bits(post[2], vo), f"{name}: moments are not the AdamW rule's"
    else:
        bref, bbound, tref, xref, bound = ref_lars(*pre, lr, wd, div, adapts)
        eb = np.abs(post[1] - bref)
        print(f"{name}: b' error / bound max {np.max(eb / np.maximum(bbound, 1e-300)):.3f}")
        assert np.all(eb <= bbound), f"{name}: momentum buffer outside its bound"
    ex = np.abs(post[0] - xref)
    print(f"{name}: trust {trust!r} ref {tref!r} ({ulps(trust, tref):.2f} ulp), "
          f"x' error / bound max {np.max(ex / np.maximum(bound, 1e-300)):.3f}")
    assert ulps(trust, tref) <= 2.0, f"{name}: trust {trust!r} vs {tref!r}"
    assert np.all(ex <= bound), f"{name}: weights outside their bound"


def make(device, kind, wd, seed=0, names=tuple(TENSORS), exempt_all=False):
    """The table's tensors as views of one flat buffer each for x and g (4 guard elements around each
    view), and the optimiser over them: ``(opt, xs, gs, adapts)``."""
    gen = torch.Generator().manual_seed(seed)
    spans, o = [], 4
    for name in names:
        n, past = TENSORS[name][:2]
        spans.append((o + past, n))
        o = (o + past + n + 3) // 4 * 4 + 4
    X = torch.zeros(o + 4)
    for (s, n), name in zip(spans, names):
        if not TENSORS[name][3]:
            X[s: s + n] = torch.randn(n, generator=gen)
    X, G = X.to(device), torch.zeros(o + 4, device=device)
    assert X.data_ptr() % 16 == 0 and G.data_ptr() % 16 == 0
    xs, gs = [X[s: s + n] for s, n in spans], [G[s: s + n] for s, n in spans]
    adapts = [TENSORS[name][2] and not exempt_all for name in names]
    if kind == "lamb":
        opt = ops.FusedLamb(xs, LR, betas=(B1, B2), eps=EPS, weight_decay=wd, adapt_mask=adapts)
    else:
        opt = ops.FusedLars(xs, LR, momentum=MU, weight_decay=wd, lars_coef=ETA, lars_eps=EPS_L, adapt_mask=adapts)
    opt.bind(gs)
    opt.flat = (X, G)
    return opt, xs, gs, adapts


def fill_grads(gs, step, names=tuple(TENSORS), scale=0.1):
    gen = torch.Generator().manual_seed(100 + step)
    for g, name in zip(gs, names):
        if not TENSORS[name][4]:
            g.copy_(torch.randn(g.numel(), generator=gen) * scale)


def state(opt):
    """The optimiser's per-tensor state as lists of float32 arrays: (m, v) or (b,)."""
    lists = (opt.exp_avg, opt.exp_avg_sq) if opt.core.lamb else (opt.momentum_buffer,)
    return [[t.detach().cpu().numpy().copy() for t in lst] for lst in lists]


def check_steps(device, kind, div, wd, steps=3):
    """``steps`` consecutive steps over the whole table, each checked on its own from the fp32 state
    before it."""
    opt, xs, gs, adapts = make(device, kind, wd)
    for k in range(steps):
        fill_grads(gs, k)
        x0 = [x.cpu().numpy().copy() for x in xs]
        g0 = [g.cpu().numpy().copy() for g in gs]
        s0 = state(opt)
        st = opt.read()
        block = (F(st["b1pow"]), F(st["b2pow"]), st["steps"]) if st else None
        opt.step(div)
        s1, trust = state(opt), opt.trust_ratios().numpy()
        assert trust.shape == (len(xs),)
        for i, name in enumerate(TENSORS):
            check_tensor(kind, f"step {k} {name}", (x0[i], g0[i], *(s[i] for s in s0)),
                         (xs[i].cpu().numpy(), *(s[i] for s in s1)), trust[i], block, LR, wd, div, adapts[i])
        if st:
            S = R.scalars(block, LR, wd, B1, B2)
            now = opt.read()
            assert (F(now["b1pow"]), F(now["b2pow"]), now["steps"]) == (S["p1"], S["p2"], st["steps"] + 1)
