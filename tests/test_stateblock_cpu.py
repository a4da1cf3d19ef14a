"""``ops.StateBlock`` without a GPU: the dict twin of the 16-byte ``{float, float, uint32, uint32}`` block.
``check_round_trip`` is shared with tests/test_stateblock_gpu.py, which runs it on a device block."""
import math

import numpy as np

from network_distributed_pytorch_amd import ops

NAMES = ("a", "b", "n", "k")
DENORMAL = float(np.float32(1e-40))  # exactly representable in fp32, below its smallest normal
assert 0.0 < DENORMAL < float(np.finfo(np.float32).tiny)
FIRST = {"a": -0.0, "b": DENORMAL, "n": 2 ** 31, "k": 2 ** 32 - 1}
SECOND = {"a": math.inf, "b": -DENORMAL, "n": 2 ** 32 - 1, "k": 2 ** 31}


def same(got, want):
    """Field by field, the sign of a zero included."""
    assert list(got) == list(want)
    for k in want:
        assert got[k] == want[k] and type(got[k]) is type(want[k]), (k, got[k], want[k])
        if isinstance(want[k], float):
            assert math.copysign(1.0, got[k]) == math.copysign(1.0, want[k]), (k, got[k], want[k])


def check_round_trip(device):
    blk = ops.StateBlock(device, NAMES, (0.0, 1.0, 0, 3))
    same(blk.read(), {"a": 0.0, "b": 1.0, "n": 0, "k": 3})  # the initial values
    blk.write(FIRST)
    same(blk.read(), FIRST)
    older = blk.snapshot()
    blk.write(SECOND)
    same(blk.read(), SECOND)
    newer = blk.snapshot()
    blk.restore(older)  # an older snapshot after a write: the older values
    same(blk.read(), FIRST)
    blk.write({"a": 2.0, "b": 3.0, "n": 1, "k": 1})
    same(blk.read(), {"a": 2.0, "b": 3.0, "n": 1, "k": 1})
    blk.restore(newer)  # a snapshot is a copy: the writes since left it alone
    same(blk.read(), SECOND)
    return blk


def test_round_trip_on_cpu():
    blk = check_round_trip("cpu")
    assert blk.dev is None  # no tensor on CPU: the twins read the dict


def test_three_fields_and_extra_keys():
    blk = ops.StateBlock("cpu", ("decay", "weight", "updates"), (0.0, 0.0, 0))
    blk.write({"decay": 0.5, "weight": 0.5, "updates": 7, "shadow": object()})  # a state dict: other keys ignored
    same(blk.read(), {"decay": 0.5, "weight": 0.5, "updates": 7})
    got = blk.read()
    got["updates"] = 99  # read() hands out a copy
    assert blk.read()["updates"] == 7


def test_the_three_owners_start_as_documented():
    import torch

    clip = ops.GradClip("cpu")
    assert clip.state.read() == {"norm": 0.0, "coef": 1.0, "clipped": 0, "steps": 0} and clip.clip is None
    ema = ops.WeightEma([torch.zeros(3)], 0.9)
    assert ema.read() == {"decay": 0.0, "weight": 0.0, "updates": 0} and ema.block is None
    opt = ops.FusedAdamW([torch.zeros(3)], 1e-3)
    assert opt.read() == {"b1pow": 1.0, "b2pow": 1.0, "steps": 0} and opt.core.block is None
    # AdamWCore.write rounds to fp32, WeightEma's load keeps what it is given
    opt.core.write({"b1pow": 0.1, "b2pow": 0.2, "steps": 4})
    assert opt.read() == {"b1pow": float(np.float32(0.1)), "b2pow": float(np.float32(0.2)), "steps": 4}
    ema.load_state_dict({"shadow": {"w": torch.ones(3)}, "decay": 0.1, "weight": 0.9, "updates": 2})
    assert ema.read() == {"decay": 0.1, "weight": 0.9, "updates": 2}
