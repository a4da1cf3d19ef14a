"""The numpy reference of tests/seg_cases.py against ``SegPlan``'s CPU path on the same inputs, the
table front end of ``SegPlan`` off the device, and the 16-byte block helpers."""
import numpy as np
import torch

from network_distributed_pytorch_amd import ops

from . import seg_cases as S


def test_numpy_reference_is_segplan_cpu_path():
    cases, src, dst = S.buffers()
    assert len(cases) == 8 * 4 * 4 * 2
    want = S.reference(cases, src, dst)
    s, d = torch.from_numpy(src.copy()), torch.from_numpy(dst.copy())
    ops.SegPlan(S.specs(cases, s, d), "cpu").run()
    assert np.array_equal(d.numpy().view(np.int32), want.view(np.int32))
    written = np.zeros(dst.size, dtype=bool)
    for c in cases:
        assert not written[c["dst"] - S.BAND: c["dst"] + c["n"] + S.BAND].any()  # bands never overlap a dst
        written[c["dst"]: c["dst"] + c["n"]] = True
    assert (want[~written] == S.SENTINEL).all() and (want[written] != S.SENTINEL).all()


def test_segplan_table_front_end_off_device():
    x = torch.arange(5.0)
    plan = ops.SegPlan([(x, torch.empty(5), 1, 0, 1.0)], "cpu")
    calls = []
    assert plan.table() is None and plan.n_blocks == 0
    assert plan.launch(lambda *a: calls.append(a)) is False and not calls


def test_block4_round_trip():
    blk = torch.zeros(4, dtype=torch.int32)
    ops.write_block4(blk, 0.999, 1e-3, 0xfffffffe, 7)
    f0, f1, u0, u1 = ops.read_block4(blk)
    assert (f0, f1) == (float(np.float32(0.999)), float(np.float32(1e-3))) and (u0, u1) == (0xfffffffe, 7)
    ops.write_block4(blk, 0.0, 0.0, 3)
    assert ops.read_block4(blk) == (0.0, 0.0, 3, 0)
