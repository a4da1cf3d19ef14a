"""The direct-conv dispatch plan (csrc/conv.hip conv_make_plan, read through the conv_plan,
conv_stats_slices, conv_dgrad_stats_slices and conv_wino bindings) against the recorded table
tests/golden/conv_plan_table.json: every shape class, near misses that must stay class -1, a ladder
of batches, Winograd on and off, every stem row-split override.  Host code only; the table was
recorded by tools/conv_plan_table.py before the dispatch was rewritten around tile descriptors."""
import json
import os

import pytest

from network_distributed_pytorch_amd.ops import native_available

pytestmark = pytest.mark.skipif(not native_available(), reason="extension not built")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan_table.json")


def test_conv_plan_table():
    from network_distributed_pytorch_amd.ops import ext
    from tools import conv_plan_table as T

    with open(GOLDEN) as fh:
        gold = json.load(fh)
    assert gold["columns"] == T.COLUMNS and gold["geoms"] == T.GEOMS
    want = gold["rows"]
    # the fixture covers the whole grid, and every class and near miss is in it
    assert len(want) == len(T.GEOMS) * len(T.BATCHES) * len(T.WINO) * len(T.PSPLIT)
    assert {r[4] for r in want} == {-1, 0, 1, 2, 3, 4, 5}
    assert all(r[4] == -1 for r in want if r[0] >= 11)
    got = T.rows(ext())  # restores the switches in a finally
    assert len(got) == len(want)
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad, f"{len(bad)} rows differ (got, want), columns {T.COLUMNS}: {bad[:5]}"
