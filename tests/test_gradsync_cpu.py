"""The ``GradSync`` contract (parallel/sync.py) on CPU: every kind ``build_grad_sync`` accepts answers every
contract method, the state round trip of the two native arms with everything attached, and ``HyperState``.

The round-trip tests use only names that exist without ``GradSync`` (``sync.opt`` / ``sync.ddp``,
``snapshot`` / ``restore``, ``set_hyper``, ``attach_ema``), so they pin the behaviour across the refactor."""
import numpy as np
import pytest
import torch

from network_distributed_pytorch_amd import ops
from network_distributed_pytorch_amd.parallel.comm import Communicator
from network_distributed_pytorch_amd.parallel.trainer import build_grad_sync

KINDS = ("powersgd", "powersgd-ref", "powersgd-api", "dense", "dense-ref", "local-sgd-nesterov", "local-adamw")
NATIVE = {"powersgd": "opt", "dense": "ddp"}  # kind -> its compatibility alias


def _mlp(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(8, 4), torch.nn.Tanh(), torch.nn.Linear(4, 2))


def _batch(k):
    g = torch.Generator().manual_seed(100 + k)
    return torch.randn(4, 8, generator=g), torch.randint(0, 2, (4,), generator=g)


def _step(sync, model, k, hyper=None):
    if hyper is not None:
        sync.set_hyper(*hyper)
    sync.zero_grad()
    x, y = _batch(k)
    torch.nn.functional.cross_entropy(model(x), y).backward()
    return sync.step()


def _bits(t):
    return t.detach().contiguous().view(torch.int32).numpy().copy()


# ---- the contract ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_every_kind_is_a_gradsync_and_answers_the_whole_contract(kind):
    from network_distributed_pytorch_amd.parallel.sync import GradSync

    model = _mlp()
    sync = build_grad_sync(kind, model, Communicator(), lr=0.05, momentum=0.9, rank=2)
    assert isinstance(sync, GradSync)
    native = kind in NATIVE
    # every contract method, called, never probed
    assert sync.plan_hyper([(0.05, 0.0), (0.04, 0.0)]) is None
    sync.set_hyper(0.05, 0.0)
    sync.prepare()
    assert _step(sync, model, 0) == 8 * sync.bytes_per_step
    sync.count_step()
    sync.check_errors()
    assert sync.clip_stats() is None  # max_grad_norm = 0
    sync.attach_ema(None)
    snap = sync.snapshot()
    sync.restore(snap)
    payloads = sync.collective_payloads()
    assert isinstance(payloads, list) and sync.collectives_per_step == 0  # one process: nothing on the wire
    sd = sync.state_dict()
    if sd is not None:
        sync.load_state_dict(sd)
    phases = sync.phases()  # last: on the native arms it switches overlap off
    # the defaults, for the arms that had no such method
    assert sync.adam_stats() is None  # SGD everywhere here
    if native:
        arena = sync.flat_weights
        assert arena is sync.x and arena.dim() == 1
        assert all(p.data_ptr() >= arena.data_ptr() and
                   p.data_ptr() + 4 * p.numel() <= arena.data_ptr() + 4 * arena.numel() for p in model.parameters())
        assert getattr(sync, NATIVE[kind]) is sync  # sync.opt / sync.ddp: the object itself
        assert isinstance(snap, dict) and phases and all(callable(fn) for fn, _ in phases)
        assert sum(payloads) >= sync.bytes_per_step > 0  # the dense buckets carry their 64-byte padding
    else:
        assert sync.flat_weights is None and snap is None and phases is None
        sync.restore(None)
    if kind.startswith("local"):
        assert payloads == [] and sync.bytes_per_step == 0 and isinstance(sd, dict)
    elif not native:
        assert sd is None and sum(payloads) == sync.bytes_per_step


def test_adam_stats_and_clip_stats_where_there_is_something_to_say():
    for kind in ("dense", "dense-ref", "powersgd-ref", "powersgd-api"):
        model = _mlp()
        sync = build_grad_sync(kind, model, Communicator(), lr=0.05, rank=2, max_grad_norm=0.5, optimizer="adamw")
        for k in range(2):
            _step(sync, model, k)
        assert sync.adam_stats()["steps"] == 2, kind
        st = sync.clip_stats()
        assert st["steps"] == 2 and st["norm"] > 0.0, kind
    with pytest.raises(AssertionError, match="max_grad_norm >= 0"):
        build_grad_sync("local-adamw", _mlp(), Communicator(), max_grad_norm=-1.0)


# ---- state round trip with everything attached (names that predate GradSync only) --------------------
def _hyper_at(k):
    return 0.05 / (1 + k), 0.01 * (1 + k % 2)  # both change from step to step


def _state(kind, sync, ema):
    eng = getattr(sync, NATIVE[kind])
    out = {"x": _bits(eng.x), "ema_arena": _bits(ema.arena), "ema": ema.read(), "clip": sync.clip_stats(),
           "step_count": eng.step_count}
    if kind == "dense":
        out.update(buf=_bits(eng.buf), v=_bits(eng.v), adam=eng.adam_stats())
    else:
        out.update(m=_bits(eng.m), e=_bits(eng.e), q=_bits(eng.buf.q_warm))
    return out


def _equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], (k, a[k], b[k])


@pytest.mark.parametrize("kind", ["dense", "powersgd"])
def test_state_round_trip_with_everything_attached(kind):
    model = _mlp(1)
    extra = {"optimizer": "adamw"} if kind == "dense" else {}  # dense: clip + EMA + AdamW; powersgd: clip + EMA
    sync = build_grad_sync(kind, model, Communicator(), lr=0.05, momentum=0.9, rank=2, max_grad_norm=0.05, **extra)
    ema = ops.WeightEma([p.detach() for p in model.parameters()], 0.9)
    sync.attach_ema(ema)
    for k in range(2):
        _step(sync, model, k, _hyper_at(k))
    snap = sync.snapshot()
    at_snap = _state(kind, sync, ema)
    for k in range(2, 4):
        _step(sync, model, k, _hyper_at(k))
    first = _state(kind, sync, ema)
    assert first["clip"]["steps"] == 4 and first["clip"]["clipped"] > 0 and first["ema"]["updates"] == 4
    assert not np.array_equal(first["x"], at_snap["x"]) and not np.array_equal(first["ema_arena"], at_snap["ema_arena"])
    sync.restore(snap)
    _equal(_state(kind, sync, ema), at_snap)
    for k in range(2, 4):
        _step(sync, model, k, _hyper_at(k))
    _equal(_state(kind, sync, ema), first)  # bitwise the first continuation


# ---- HyperState on CPU --------------------------------------------------------------------------------
def test_hyper_state_rounds_keeps_the_decay_and_plans_nothing_without_a_block():
    from network_distributed_pytorch_amd.ops.hyper import HyperState
    from network_distributed_pytorch_amd.parallel.ddp import BucketedDataParallel
    from network_distributed_pytorch_amd.parallel.powersgd import PowerSGDOptimizer

    f32 = lambda v: float(np.float32(v))  # noqa: E731
    assert f32(0.1) != 0.1 and f32(0.3) != 0.3
    arms = [ops.FusedAdamW([torch.zeros(3)], 0.1, weight_decay=0.3),
            BucketedDataParallel(_mlp(), Communicator(), lr=0.1, weight_decay=0.3),
            PowerSGDOptimizer(_mlp().parameters(), lr=0.1, rank=2, weight_decay=0.3)]
    # construction: FusedAdamW rounds, the two syncs keep the value they were given
    assert (arms[0].lr, arms[0].weight_decay) == (f32(0.1), f32(0.3))
    assert all((a.lr, a.weight_decay) == (0.1, 0.3) for a in arms[1:])
    for a in arms:
        assert isinstance(a, HyperState) and a.hyper is None and not a._hyper_on  # CPU: no block, nothing uploaded
        assert a.plan_hyper([(0.2, 0.0), (0.1, 0.0)]) is None
        a.set_hyper(0.2)  # None keeps the decay, rounded to fp32 like the rate
        assert (a.lr, a.weight_decay) == (f32(0.2), f32(0.3))
        a.set_hyper(0.7, 0.6)
        assert (a.lr, a.weight_decay) == (f32(0.7), f32(0.6)) and a.hyper is None and not a._hyper_on
        with pytest.raises(AssertionError, match="weight_decay"):
            a.set_hyper(0.1, -1.0)
        assert (a.lr, a.weight_decay) == (f32(0.7), f32(0.6))
