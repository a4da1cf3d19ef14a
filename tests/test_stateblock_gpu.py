"""``ops.StateBlock`` on a device: the round trip of tests/test_stateblock_cpu.py through the ``int32[4]``
tensor, which is allocated at construction and is the one handed to kernels ever after.  No launch."""
import pytest
import torch

from network_distributed_pytorch_amd import ops

from .test_stateblock_cpu import NAMES, check_round_trip

pytestmark = pytest.mark.gpu


def test_round_trip_on_the_device_block(device):
    probe = ops.StateBlock(device, NAMES, (0.0, 1.0, 0, 3))
    dev, ptr = probe.dev, probe.dev.data_ptr()
    assert dev.dtype == torch.int32 and tuple(dev.shape) == (4,) and dev.device == device
    blk = check_round_trip(device)  # write / read / snapshot / restore, edge values included
    assert blk.dev.dtype == torch.int32 and tuple(blk.dev.shape) == (4,)
    # the tensor of construction is still the block after write and restore
    snap = probe.snapshot()
    probe.write({"a": -0.0, "b": 2.5, "n": 2 ** 31, "k": 2 ** 32 - 1})
    assert probe.dev is dev and probe.dev.data_ptr() == ptr
    assert snap.data_ptr() != ptr  # a snapshot is a copy
    probe.restore(snap)
    assert probe.dev is dev and probe.dev.data_ptr() == ptr
    assert probe.read() == {"a": 0.0, "b": 1.0, "n": 0, "k": 3}
    # the owners hand kernels that very tensor under their documented names
    clip = ops.GradClip(device)
    assert clip.clip is clip.state.dev and ops.read_block4(clip.clip) == (0.0, 1.0, 0, 0)
    ema = ops.WeightEma([torch.zeros(4, device=device)], 0.9)
    assert ema.block is ema.state.dev and ops.read_block4(ema.block) == (0.0, 0.0, 0, 0)
    core = ops.FusedAdamW([torch.zeros(4, device=device)], 1e-3).core
    assert core.block is core.state.dev and ops.read_block4(core.block) == (1.0, 1.0, 0, 0)
