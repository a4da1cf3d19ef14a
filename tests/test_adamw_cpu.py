"""Fused AdamW without a GPU: the torch twin and ``adamw_scalars`` against the test-only rule
(tests/adamw_rule.py), the condition on the GPU test's inputs (they tell the rule from its contracted
variants), the accuracy against ``torch.optim.AdamW`` in fp64, the config keys, the gradient syncs,
the engine on the CPU MLP task and two gloo ranks."""
import json
import os

import numpy as np
import pytest
import torch

from network_distributed_pytorch_amd import engine, ops
from network_distributed_pytorch_amd.parallel import trainer
from network_distributed_pytorch_amd.parallel.comm import Communicator
from network_distributed_pytorch_amd.parallel.ddp import BucketedDataParallel
from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync
from network_distributed_pytorch_amd.utils.config import ConfigError, validate_config
from network_distributed_pytorch_amd.utils.launcher import spawn

from . import adamw_cases as C
from . import adamw_dist_helpers as H
from . import adamw_rule as R

F = np.float32


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().view(torch.int32).numpy().copy()  # the engine picks a device when there is one


# ---- twin against the rule -----------------------------------------------------------------------
@pytest.mark.parametrize("div", [1.0, 3.0])
@pytest.mark.parametrize("wd", [0.0, 0.05])
def test_twin_equals_rule(div, wd):
    shapes = [(5,), (3, 7), (), (301,), (2, 3, 4)]
    mask = [True, False, True, False, True]  # both decay flags
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    xs = [torch.from_numpy(R.gaussians(10 + i, int(np.prod(s, dtype=np.int64))).reshape(s)) for i, s in enumerate(shapes)]
    x0 = [x.numpy().copy() for x in xs]
    opt = ops.FusedAdamW(xs, lr, betas=(b1, b2), eps=eps, weight_decay=wd, decay_mask=mask)
    assert opt.read() == {"b1pow": 1.0, "b2pow": 1.0, "steps": 0}
    assert all(float(m.abs().sum()) == 0.0 and float(v.abs().sum()) == 0.0 for m, v in zip(opt.exp_avg, opt.exp_avg_sq))
    gs = [[R.gaussians(1000 * k + i, x.numel(), 1e-2) for i, x in enumerate(xs)] for k in range(3)]
    ref = [R.run(x0[i], [gs[k][i] for k in range(3)], lr, wd, b1, b2, eps, div, mask[i]) for i in range(len(xs))]
    grads = [torch.zeros_like(x) for x in xs]
    opt.bind(grads)
    for k in range(3):
        for g, a in zip(grads, gs[k]):
            g.copy_(torch.from_numpy(a).view_as(g))
        keep = [_bits(g) for g in grads]
        opt.step(div)
        assert all(np.array_equal(_bits(g), b) for g, b in zip(grads, keep))  # the gradient is only read
        for i in range(len(xs)):
            x, m, v, blk = ref[i][k]
            assert R.same_bits(xs[i].numpy().ravel(), x), (i, k)
            assert R.same_bits(opt.exp_avg[i].numpy().ravel(), m), (i, k)
            assert R.same_bits(opt.exp_avg_sq[i].numpy().ravel(), v), (i, k)
        blk = ref[0][k][3]
        assert opt.read() == {"b1pow": float(blk[0]), "b2pow": float(blk[1]), "steps": k + 1}
    if wd:  # the decay flag matters: the exempt tensors equal a wd = 0 run, the others do not
        nodecay = R.run(x0[1], [gs[k][1] for k in range(3)], lr, 0.0, b1, b2, eps, div, True)
        assert R.same_bits(xs[1].numpy().ravel(), nodecay[-1][0])
        plain = R.run(x0[0], [gs[k][0] for k in range(3)], lr, 0.0, b1, b2, eps, div, True)
        assert not R.same_bits(xs[0].numpy().ravel(), plain[-1][0])


def test_special_values_twin_equals_rule_and_documented_consequences():
    x, g, m, v = C.specials()
    for wd in (0.0, 0.05):
        opt = ops.FusedAdamW([torch.from_numpy(x.copy())], 1e-3, weight_decay=wd)
        opt.exp_avg[0].copy_(torch.from_numpy(m))
        opt.exp_avg_sq[0].copy_(torch.from_numpy(v))
        opt.bind([torch.from_numpy(g.copy())])
        opt.step()
        rx, rm, rv, _ = R.step(x, g, m, v, (F(1), F(1), 0), 1e-3, wd, 0.9, 0.999, 1e-8)
        assert R.same_bits(opt.params[0].numpy(), rx)
        assert R.same_bits(opt.exp_avg[0].numpy(), rm) and R.same_bits(opt.exp_avg_sq[0].numpy(), rv)
        if wd == 0.0:  # g = m = v = 0 keeps x, -0 included (rows 0 and 1 of the specials)
            assert rx[0] == 0 and not np.signbit(rx[0]) and rx[1] == 0 and np.signbit(rx[1])
        assert np.isnan(rx[np.isnan(g)]).all()


def test_step_arrays_is_the_scalar_loop():
    x, g, m, v = (R.gaussians(s, 257) for s in (1, 2, 3, 4))
    v = np.abs(v)
    blk = (F(0.9), F(0.999), 1)
    for con in (None,) + R.CONTRACTED:
        a = R.step(x, g, m, v, blk, 1e-3, 0.05, 0.9, 0.999, 1e-8, 3.0, True, con)
        b = R.step_arrays(x, g, m, v, blk, 1e-3, 0.05, 0.9, 0.999, 1e-8, 3.0, True, con)
        assert all(R.same_bits(p, q) for p, q in zip(a[:3], b[:3])) and a[3] == b[3]


# ---- the GPU test's inputs tell the rule from each contracted variant ----------------------------
def test_gpu_inputs_discriminate_contracted_variants():
    tables = [C.main_table()] + [C.one_entry(n) for n in C.ONE_ENTRY]
    for cases in tables:
        bufs = C.buffers(cases)
        gbuf, gst = bufs["g"]
        for div, wd in ((1.0, 0.0), (3.0, C.WD)):
            differs = {c: 0 for c in R.CONTRACTED}
            for ci, case in enumerate(cases):
                n, dec = case[0], case[4]
                if n > 5000 and len(cases) > 1 and n != C.BIG:
                    continue
                x = bufs["x"][0][bufs["x"][1][ci]: bufs["x"][1][ci] + n]
                st = {c: (x, np.zeros(n, F), np.zeros(n, F), (F(1), F(1), 0)) for c in (None,) + R.CONTRACTED}
                gk = gbuf
                for k in range(3):
                    if k:
                        gk = C.next_grads(gbuf, cases, gst, k)
                    g = gk[gst[ci]: gst[ci] + n]
                    assert np.all(np.isfinite(g)) and np.all(np.abs(g) >= np.finfo(F).tiny)
                    for c in st:
                        st[c] = R.step_arrays(st[c][0], g, st[c][1], st[c][2], st[c][3], C.LR, wd, C.BETA1, C.BETA2,
                                              C.EPS, div, dec, c)
                for c in R.CONTRACTED:
                    differs[c] += sum(int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32)))
                                      for a, b in zip(st[c][:3], st[None][:3]))
            assert all(k > 0 for k in differs.values()), (len(cases), div, wd, differs)


# ---- the schedule twin ---------------------------------------------------------------------------
def test_adamw_scalars_against_the_block():
    b1, b2, lr, wd = 0.9, 0.999, 3e-4, 0.01
    opt = ops.FusedAdamW([torch.ones(3)], lr, betas=(b1, b2), weight_decay=wd)
    opt.bind([torch.ones(3)])
    blk = (F(1.0), F(1.0), 0)
    for k in range(60):
        S, got = R.scalars(blk, lr, wd, b1, b2), ops.adamw_scalars(blk[0], blk[1], lr, wd, b1, b2)
        assert sorted(S) == sorted(got)
        for key in S:
            assert isinstance(got[key], np.float32) and got[key].tobytes() == S[key].tobytes(), (k, key)
        opt.step()
        blk = (S["p1"], S["p2"], k + 1)
        assert opt.read() == {"b1pow": float(S["p1"]), "b2pow": float(S["p2"]), "steps": k + 1}
    # the running product against the power it replaces: within a few ulp after 60 multiplies
    assert abs(float(blk[0]) - 0.9 ** 60) < 60 * 2.0 ** -24 * 0.9 ** 60 * 2
    assert ops.adamw_scalars(1.0, 1.0, lr, 0.0, 0.0, 0.0)["ss"] == F(lr)  # beta = 0: no correction


# ---- against torch.optim.AdamW -------------------------------------------------------------------
def _prototype_grads(seed, n, steps):
    """Gaussian gradients with per-element magnitudes from 1e-4 to 10 (log-uniform)."""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.uniform(-4.0, 1.0, n)
    return [(rng.standard_normal(n) * mag).astype(F) for _ in range(steps)], rng.standard_normal(n).astype(F)


def _torch_adamw(x0, gs, lr, wd, dtype, groups=None, betas=(0.9, 0.999), eps=1e-8):
    ps = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(dtype)) for a in x0]
    if groups is None:
        opt = torch.optim.AdamW(ps, lr=lr, betas=betas, eps=eps, weight_decay=wd)
    else:
        opt = torch.optim.AdamW([{"params": [p for p, d in zip(ps, groups) if d], "weight_decay": wd},
                                 {"params": [p for p, d in zip(ps, groups) if not d], "weight_decay": 0.0}],
                                lr=lr, betas=betas, eps=eps)
    for step in gs:
        for p, g in zip(ps, step):
            p.grad = torch.from_numpy(g.copy()).to(dtype).view_as(p)
        opt.step()
    return [p.detach().double().numpy().ravel() for p in ps]


@pytest.mark.parametrize("lr,wd", [(5e-5, 0.0), (1e-3, 0.01), (1e-2, 0.1)])
def test_twin_is_as_close_to_fp64_adamw_as_torch_fp32(lr, wd):
    for seed in range(5):
        gs, x0 = _prototype_grads(seed, 256, 200)
        x = torch.from_numpy(x0.copy())
        opt = ops.FusedAdamW([x], lr, weight_decay=wd)
        g = torch.zeros(256)
        opt.bind([g])
        for a in gs:
            g.copy_(torch.from_numpy(a))
            opt.step()
        ref = _torch_adamw([x0], [[a] for a in gs], lr, wd, torch.float64)[0]
        e32 = float(np.abs(_torch_adamw([x0], [[a] for a in gs], lr, wd, torch.float32)[0] - ref).max())
        etw = float(np.abs(x.double().numpy() - ref).max())
        print(f"lr={lr} wd={wd} seed={seed}: twin max abs err {etw:.3e}, torch fp32 {e32:.3e}, ratio {etw / e32:.3f}")
        assert opt.read()["steps"] == 200
        assert e32 > 0 and etw <= 1.5 * e32


def test_decay_1d_false_equals_two_torch_param_groups():
    lr, wd, steps = 1e-3, 0.1, 200
    torch.manual_seed(5)
    model = H.make_model()
    ps = list(model.parameters())
    x0 = [p.detach().numpy().copy() for p in ps]
    groups = [p.dim() > 1 for p in ps]
    assert groups == [True, False, True, False]
    rng = np.random.default_rng(11)
    gs = [[(rng.standard_normal(p.numel()) * 10.0 ** rng.uniform(-4, 1, p.numel())).astype(F) for p in ps]
          for _ in range(steps)]
    sync = build_grad_sync("dense", model, Communicator(), lr=lr, optimizer="adamw", decay_1d=False)
    sync.set_hyper(lr, wd)
    for step in gs:
        sync.zero_grad()
        for p, g in zip(ps, step):
            p.grad = torch.from_numpy(g.copy()).view_as(p)
        sync.step()
    assert sync.adam_stats()["steps"] == steps and len(sync.ddp.adam_runs) == 4
    ref = _torch_adamw(x0, gs, lr, wd, torch.float64, groups)
    t32 = _torch_adamw(x0, gs, lr, wd, torch.float32, groups)
    e32 = max(float(np.abs(a - b).max()) for a, b in zip(t32, ref))
    etw = max(float(np.abs(p.detach().double().numpy().ravel() - b).max()) for p, b in zip(ps, ref))
    print(f"decay_1d=False: sync max abs err {etw:.3e}, torch fp32 {e32:.3e}, ratio {etw / e32:.3f}")
    assert e32 > 0 and etw <= 1.5 * e32
    # ... and decaying everything is a different run on the 1-D tensors
    alld = _torch_adamw(x0, gs, lr, wd, torch.float64)
    assert float(np.abs(alld[1] - ref[1]).max()) > 100 * e32
    # dense-ref, the comparison arm: torch.optim.AdamW with the same two groups
    torch.manual_seed(5)
    model2 = H.make_model()
    ref_sync = build_grad_sync("dense-ref", model2, Communicator(), lr=lr, optimizer="adamw", decay_1d=False)
    ref_sync.set_hyper(lr, wd)
    assert [g["weight_decay"] for g in ref_sync.opt.param_groups] == [wd, 0.0]
    assert [len(g["params"]) for g in ref_sync.opt.param_groups] == [2, 2]
    for step in gs[:5]:
        ref_sync.zero_grad()
        for p, g in zip(model2.parameters(), step):
            p.grad = torch.from_numpy(g.copy()).view_as(p)
        ref_sync.step()
    assert ref_sync.adam_stats() == {"steps": 5}
    five = _torch_adamw(x0, gs[:5], lr, wd, torch.float32, groups)
    assert all(np.array_equal(p.detach().double().numpy().ravel(), a) for p, a in zip(model2.parameters(), five))


# ---- config, CLI -----------------------------------------------------------------------------------
def test_config_keys_and_errors():
    c = validate_config({})
    d = engine.default_config()
    for cfg in (c, d):
        assert (cfg["optimizer"], cfg["adam_beta1"], cfg["adam_beta2"], cfg["adam_eps"], cfg["decay_1d"]) == \
            ("sgd", 0.9, 0.999, 1e-8, True)
    c = validate_config({"optimizer": "adamw", "grad_sync": "dense", "adam_beta1": 0.8, "adam_beta2": 0.0,
                         "adam_eps": 1e-6, "decay_1d": 0})
    assert c["optimizer"] == "adamw" and c["decay_1d"] is False and c["adam_beta2"] == 0.0
    nan, inf = float("nan"), float("inf")
    for key in ("adam_beta1", "adam_beta2"):
        for bad in (-0.1, 1.0, 1.5, nan, inf, 1.0 - 1e-12):
            with pytest.raises(ConfigError, match=key):
                validate_config({key: bad})
    for bad in (0.0, -1e-8, nan, inf, 1e-60):
        with pytest.raises(ConfigError, match="adam_eps"):
            validate_config({"adam_eps": bad})
    for bad in ("adam", "AdamW", ""):
        with pytest.raises(ConfigError, match="optimizer"):
            validate_config({"optimizer": bad})
    with pytest.raises(ConfigError, match="optimizer"):
        validate_config({"optimizer": None})
    for sync in ("powersgd", "local-sgd-nesterov", "local-adamw"):
        with pytest.raises(ConfigError, match="adamw"):
            validate_config({"optimizer": "adamw", "grad_sync": sync})
        validate_config({"optimizer": "sgd", "grad_sync": sync})
    for sync in ("dense", "dense-ref", "powersgd-ref", "powersgd-api"):
        validate_config({"optimizer": "adamw", "grad_sync": sync})
    from network_distributed_pytorch_amd.workloads import _cli

    a = _cli.build_parser(1).parse_args(["-optimizer", "adamw", "-adam_beta1", "0.8", "-adam_beta2", "0.98",
                                         "-adam_eps", "1e-6", "-decay_1d", "0"])
    assert (a.optimizer, a.adam_beta1, a.adam_beta2, a.adam_eps, a.decay_1d) == ("adamw", 0.8, 0.98, 1e-6, 0)
    a = _cli.build_parser(1).parse_args([])
    assert a.optimizer is None and a.adam_beta1 is None and a.decay_1d is None


def test_argument_checks():
    x = torch.zeros(4)
    for bad in ((1.0, 0.9), (0.9, 1.0), (-0.1, 0.9), (float("nan"), 0.9), (0.9,)):
        with pytest.raises(ValueError):
            ops.FusedAdamW([x], 1e-3, betas=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError, match="eps"):
            ops.FusedAdamW([x], 1e-3, eps=bad)
    with pytest.raises(ValueError, match="float32"):
        ops.FusedAdamW([torch.zeros(3, dtype=torch.float64)], 1e-3)
    with pytest.raises(ValueError, match="contiguous"):
        ops.FusedAdamW([torch.zeros(4, 4).t()], 1e-3)
    with pytest.raises(ValueError, match="decay_mask"):
        ops.FusedAdamW([x], 1e-3, decay_mask=[True, False])
    with pytest.raises(ValueError, match="no parameters"):
        ops.FusedAdamW([], 1e-3)
    opt = ops.FusedAdamW([x], 1e-3)
    with pytest.raises(RuntimeError, match="bind"):
        opt.step()
    with pytest.raises(ValueError):
        opt.bind([])
    with pytest.raises(ValueError, match="float32"):
        opt.bind([torch.zeros(4, dtype=torch.float64)])
    with pytest.raises(ValueError, match="elements"):
        opt.bind([torch.zeros(5)])
    with pytest.raises(ValueError, match="None"):
        opt.bind([None])
    opt.bind([torch.zeros(4)])
    with pytest.raises(ValueError, match="div"):
        opt.step(0.5)


def test_moments_follow_parameter_alignment():
    base = torch.zeros(64)
    xs = [base[1:6], base[8:12], base[12:20], torch.ones(3, 2)]  # 4 B past, aligned, adjacent, own storage
    opt = ops.FusedAdamW(xs, 1e-3)
    for x, m, v in zip(xs, opt.exp_avg, opt.exp_avg_sq):
        assert m.data_ptr() % 16 == x.data_ptr() % 16 and v.data_ptr() % 16 == x.data_ptr() % 16
        assert m.shape == x.shape and v.shape == x.shape
    assert opt.offsets[2] == opt.offsets[1] + 4  # adjacent parameters: adjacent moments


# ---- build_grad_sync ---------------------------------------------------------------------------------
def test_build_grad_sync_pass_through_and_unchanged_sgd_call(monkeypatch):
    calls = []

    def rec(name):
        def ctor(*a, **kw):
            calls.append((name, a[2:], kw))
            return name
        return ctor
    for name in ("PowerSGDSync", "ReferencePowerSGDLoop", "_DenseSync", "ReferenceDenseLoop", "LocalOptimizer"):
        monkeypatch.setattr(trainer, name, rec(name))
    comm, model = object(), object()
    # optimizer="sgd" (given or not): every constructor call exactly what it is without the feature
    for kw in ({}, {"optimizer": "sgd", "betas": (0.5, 0.5), "eps": 1.0, "decay_1d": False}):
        calls.clear()
        for kind in ("powersgd", "powersgd-ref", "powersgd-api", "dense", "dense-ref", "local-adamw"):
            build_grad_sync(kind, model, comm, lr=0.1, momentum=0.8, rank=3, bucket_mb=2.0, seed=5, **kw)
        assert calls == [("PowerSGDSync", (0.1, 0.8, 3), {"seed": 5}),
                         ("ReferencePowerSGDLoop", (0.1, 0.8, 3), {"seed": 5}),
                         ("ReferencePowerSGDLoop", (0.1, 0.8, 3), {"seed": 5, "native_reducer": True}),
                         ("_DenseSync", (0.1, 0.8, 2.0), {"overlap": None}),
                         ("ReferenceDenseLoop", (0.1, 0.8), {}),
                         ("LocalOptimizer", (0.1, 0.8), {})]  # (model, kind, lr, momentum)
    adam = {"optimizer": "adamw", "betas": (0.8, 0.98), "eps": 1e-6, "decay_1d": False}
    calls.clear()
    for kind in ("powersgd-ref", "powersgd-api", "dense", "dense-ref"):
        build_grad_sync(kind, model, comm, lr=0.1, momentum=0.8, rank=3, bucket_mb=2.0, seed=5, max_grad_norm=1.0, **adam)
    clip = {"max_grad_norm": 1.0}
    assert calls == [("ReferencePowerSGDLoop", (0.1, 0.8, 3), {"seed": 5, **clip, **adam}),
                     ("ReferencePowerSGDLoop", (0.1, 0.8, 3), {"seed": 5, "native_reducer": True, **clip, **adam}),
                     ("_DenseSync", (0.1, 0.8, 2.0), {"overlap": None, **clip, **adam}),
                     ("ReferenceDenseLoop", (0.1, 0.8), {**clip, **adam})]
    for kind in ("powersgd", "local-sgd-nesterov", "local-adamw"):
        with pytest.raises(ValueError, match="no AdamW"):
            build_grad_sync(kind, model, comm, optimizer="adamw")
    with pytest.raises(ValueError, match="unknown optimizer"):
        build_grad_sync("dense", model, comm, optimizer="lamb")
    with pytest.raises(ValueError, match="beta"):
        build_grad_sync("dense", model, comm, optimizer="adamw", betas=(1.0, 0.9))


# ---- state --------------------------------------------------------------------------------------------
def _some_steps(sync, model, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    for _ in range(n):
        sync.zero_grad()
        x = torch.randn(8, 12, generator=g)
        y = torch.randint(0, 5, (8,), generator=g)
        torch.nn.functional.cross_entropy(model(x), y).backward()
        sync.step()


def test_state_dict_round_trip_and_optimizer_mismatch():
    torch.manual_seed(2)
    xs = [torch.randn(7), torch.randn(3, 5)]
    opt = ops.FusedAdamW(xs, 1e-2, weight_decay=0.1, decay_mask=[False, True])
    grads = [torch.randn(7), torch.randn(3, 5)]
    opt.bind(grads)
    for _ in range(3):
        opt.step()
    sd = opt.state_dict()
    assert sd["steps"] == 3 and len(sd["exp_avg"]) == 2 and sd["betas"] == (0.9, 0.999)
    snap = opt.snapshot()
    before = [x.clone() for x in xs]
    opt.step()
    after = [x.clone() for x in xs]
    opt.restore(snap)
    assert opt.read()["steps"] == 3 and all(torch.equal(a, b) for a, b in zip(sd["exp_avg_sq"], opt.exp_avg_sq))
    other = ops.FusedAdamW([b.clone() for b in before], 5.0, decay_mask=[False, True])
    other.load_state_dict(sd)
    assert other.read() == opt.read() and other.lr == opt.lr and other.weight_decay == opt.weight_decay
    other.bind(grads)
    other.step()
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(other.params, after))
    with pytest.raises(ValueError):
        ops.FusedAdamW([torch.zeros(7)], 1e-2).load_state_dict(sd)
    # the dense sync: AdamW and SGD checkpoints do not load into each other
    torch.manual_seed(3)
    ma, ms = H.make_model(), H.make_model()
    a = BucketedDataParallel(ma, Communicator(), lr=1e-2, optimizer="adamw", weight_decay=0.1)
    s = BucketedDataParallel(ms, Communicator(), lr=1e-2)
    _some_steps(a, ma, 3)
    _some_steps(s, ms, 3)
    sa, ss = a.state_dict(), s.state_dict()
    assert sa["optimizer"] == "adamw" and sa["steps"] == 3 and "exp_avg_sq" in sa and "optimizer" not in ss
    assert sorted(ss) == ["lr", "momentum", "momentum_buffer", "weight_decay"]  # the SGD checkpoint is what it was
    with pytest.raises(ValueError, match="sgd optimizer state.*adamw"):
        a.load_state_dict(ss)
    with pytest.raises(ValueError, match="adamw optimizer state.*sgd"):
        s.load_state_dict(sa)
    torch.manual_seed(3)
    mb = H.make_model()
    H.make_model()
    b = BucketedDataParallel(mb, Communicator(), lr=1.0, optimizer="adamw")
    b.x.copy_(a.x)
    b.load_state_dict(sa)
    assert b.adam_stats() == a.adam_stats() and b.lr == a.lr and b.weight_decay == a.weight_decay
    snap = a.snapshot()
    _some_steps(a, ma, 2, seed=9)
    _some_steps(b, mb, 2, seed=9)
    assert np.array_equal(_bits(a.x), _bits(b.x)) and np.array_equal(_bits(a.v), _bits(b.v))
    assert a.adam_stats()["steps"] == 5
    a.restore(snap)  # a graph warm-up leaves no trace: v and the block come back
    assert a.adam_stats()["steps"] == 3 and torch.equal(a.v, sa["exp_avg_sq"]) and torch.equal(a.buf, sa["momentum_buffer"])


# ---- two gloo ranks -----------------------------------------------------------------------------------
@pytest.mark.parametrize("decay_1d", [True, False])
def test_two_ranks_equal_the_twin_on_averaged_gradients(tmp_path, decay_1d):
    steps = 4
    spawn(H.adamw_rank_body, 2, args=(str(tmp_path), steps, decay_1d))
    a, b = (torch.load(os.path.join(tmp_path, f"adamw_rank{r}.pt"), weights_only=True) for r in range(2))
    assert a["block"] == b["block"] and a["block"]["steps"] == steps
    for p, q in zip(a["params"], b["params"]):
        assert np.array_equal(_bits(p), _bits(q))  # replicas identical
    for (m0, v0), (m1, v1) in zip(a["moments"], b["moments"]):
        assert np.array_equal(_bits(m0), _bits(m1)) and np.array_equal(_bits(v0), _bits(v1))
    assert all(torch.equal(p, q) for p, q in zip(a["init"], b["init"]))  # broadcast from rank 0
    assert any(not torch.equal(g, h) for g, h in zip(a["grads"][0], b["grads"][0]))
    xs = [p.clone() for p in a["init"]]
    opt = ops.FusedAdamW(xs, H.LR, betas=H.BETAS, eps=H.EPS, weight_decay=H.WD,
                         decay_mask=[decay_1d or p.dim() > 1 for p in xs])
    for k in range(steps):
        opt.bind([(g + h) / 2 for g, h in zip(a["grads"][k], b["grads"][k])])  # N = 2 divides exactly
        opt.step()
    assert opt.read() == a["block"]
    for x, p, (m, v), em, ev in zip(xs, a["params"], a["moments"], opt.exp_avg, opt.exp_avg_sq):
        assert np.array_equal(_bits(x), _bits(p))
        assert np.array_equal(_bits(em), _bits(m)) and np.array_equal(_bits(ev), _bits(v))
        assert not torch.equal(x, a["init"][0]) if x.shape == a["init"][0].shape else True


# ---- the engine on the CPU MLP task -----------------------------------------------------------------
def _run(tmp_path, name, grad_sync="dense", epochs=2, **kw):
    cfg = engine.default_config(task="mlp", grad_sync=grad_sync, dataset_size=256, global_batch=32,
                                training_epochs=epochs, verbose=False, learning_rate=0.01,
                                log_file=str(tmp_path / f"{name}.jsonl"), **kw)
    torch.manual_seed(1)
    out = engine.run_task(cfg)
    recs = [json.loads(ln) for ln in (tmp_path / f"{name}.jsonl").read_text().splitlines()]
    return out, recs


ADAM = dict(optimizer="adamw", lr_schedule="cosine", lr_warmup_steps=2, weight_decay=0.05, decay_1d=False)


def test_engine_records_and_resume_bitwise(tmp_path, monkeypatch):
    real_save = engine.save_checkpoint

    def save_every_epoch(path, model, sync, epoch, **kw):  # the mid-run checkpoint survives the later epochs
        real_save(path, model, sync, epoch=epoch, **kw)
        real_save(os.path.join(os.path.dirname(path), f"epoch{epoch}.pt"), model, sync, epoch=epoch, **kw)
    monkeypatch.setattr(engine, "save_checkpoint", save_every_epoch)
    sgd, recs_sgd = _run(tmp_path, "sgd")
    assert not any("optimizer" in r or "adam_steps" in r for r in recs_sgd) and "optimizer" not in sgd
    ck = tmp_path / "ck"
    full, recs = _run(tmp_path, "full", checkpoint_dir=str(ck), **ADAM)
    assert full["steps"] == 16 and full["optimizer"] == "adamw" and full["adam_steps"] == 16
    assert [r["adam_steps"] for r in recs if r["kind"] == "epoch"] == [8, 16]
    assert all(r["optimizer"] == "adamw" for r in recs if r["kind"] in ("epoch", "summary"))
    assert not any("optimizer" in r for r in recs if r["kind"] == "step")
    assert full["param_checksum"] != sgd["param_checksum"] and np.isfinite(full["epoch_losses"]).all()
    assert full["epoch_losses"][1] < full["epoch_losses"][0]
    state = torch.load(ck / "epoch0.pt", map_location="cpu", weights_only=True)  # plain tensors and containers
    assert state["sync"]["optimizer"] == "adamw" and state["sync"]["steps"] == 8
    torch.manual_seed(99)  # the resumed run's initialisation is replaced by the checkpoint
    res, _ = _run(tmp_path, "resumed", resume=str(ck / "epoch0.pt"), **ADAM)
    assert res["adam_steps"] == 16 and res["sync"].adam_stats() == full["sync"].adam_stats()
    for a, b in zip(full["model"].parameters(), res["model"].parameters()):
        assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(_bits(full["sync"].ddp.buf), _bits(res["sync"].ddp.buf))
    assert np.array_equal(_bits(full["sync"].ddp.v), _bits(res["sync"].ddp.v))
    # an SGD checkpoint into an AdamW run says what is wrong
    ck2 = tmp_path / "ck2"
    _run(tmp_path, "plain", epochs=1, checkpoint_dir=str(ck2))
    with pytest.raises(ValueError, match="sgd optimizer state"):
        _run(tmp_path, "bad", resume=str(ck2 / "epoch0.pt"), **ADAM)


@pytest.mark.parametrize("grad_sync", ["dense-ref", "powersgd-ref", "powersgd-api"])
def test_engine_other_arms_run_adamw(tmp_path, grad_sync):
    # the reference PowerSGD loops run eagerly (their reducer's torch path uploads inside the step)
    mode = "auto" if grad_sync == "dense-ref" else "none"
    out, recs = _run(tmp_path, "o", grad_sync, epochs=1, optimizer="adamw", weight_decay=0.01, graph_mode=mode)
    assert out["steps"] == 8 and np.isfinite(out["epoch_losses"]).all()
    # dense-ref keeps no snapshot: where its step is captured, the warm-up steps count too
    assert out["adam_steps"] == 8 if out["graph_mode"] == "none" else out["adam_steps"] > 8
    with pytest.raises(ConfigError, match="adamw"):
        _run(tmp_path, "p", "powersgd", optimizer="adamw")


# ---- PowerSGD-compressed Adam: memory and wire untouched -------------------------------------------
@pytest.mark.parametrize("kind", ["powersgd-ref", "powersgd-api"])
def test_powersgd_ref_adamw_leaves_error_memory_and_wire_alone(kind):
    def first_step(**kw):
        torch.manual_seed(4)
        model = H.make_model()
        comm = Communicator()
        sync = build_grad_sync(kind, model, comm, lr=0.01, momentum=0.9, rank=2, **kw)
        g = torch.Generator().manual_seed(3)
        x, y = torch.randn(16, 12, generator=g), torch.randint(0, 5, (16,), generator=g)
        sync.zero_grad()
        torch.nn.functional.cross_entropy(model(x), y).backward()
        bits = sync.step()
        return sync, model, bits
    s, ms, bits_s = first_step()
    a, ma, bits_a = first_step(optimizer="adamw", decay_1d=False)
    assert bits_a == bits_s and a.bytes_per_step == s.bytes_per_step and a.collective_payloads() == s.collective_payloads()
    for e, f in zip(s.memories, a.memories):
        assert np.array_equal(_bits(e), _bits(f))
    assert any(float(e.abs().max()) > 0 for e in a.memories)
    assert a.adam_stats()["steps"] == 1 and s.adam_stats() is None
    assert any(not torch.equal(p, q) for p, q in zip(ms.parameters(), ma.parameters()))  # another update rule
    # the update is the twin's on the decompressed gradients the reducer left in .grad
    torch.manual_seed(4)
    fresh = H.make_model()
    opt = ops.FusedAdamW([p.detach() for p in fresh.parameters()], 0.01, decay_mask=[p.dim() > 1 for p in fresh.parameters()])
    opt.bind([p.grad for p in ma.parameters()])
    opt.step()
    for p, q in zip(fresh.parameters(), ma.parameters()):
        assert np.array_equal(_bits(p), _bits(q))
