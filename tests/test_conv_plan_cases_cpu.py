"""tests/conv_plan_cases.py reaches every direct-conv plan of the recorded table: the cases that
tests/test_conv_plans_gpu.py runs against fp64 leave no plan key out, and (with the extension built)
the bindings still report each case's row under the case's switches.  Host code only.  If
tests/golden/conv_plan_table.json is regenerated and the counts move, the numbers here move with it,
in the same commit as the new fixture."""
import collections

import pytest

from network_distributed_pytorch_amd.ops import native_available
from tests import conv_plan_cases as R
from tools import conv_plan_table as T

N_KEYS = 136
N_CASES = 232
BY_CLASS = {0: 42, 1: 44, 2: 44, 3: 30, 4: 40, 5: 32}  # cases per class
COL = {c: i for i, c in enumerate(T.COLUMNS)}


def test_cases_cover_every_plan_key():
    cases = R.cases()
    keys = R.all_keys()
    assert len(keys) == N_KEYS and len(cases) == N_CASES
    assert {c.key for c in cases} == keys  # no key is exempt
    assert len({c.id for c in cases}) == N_CASES, "ids must tell the cases apart"
    assert cases == R.cases.__wrapped__()  # deterministic
    assert collections.Counter(c.cls for c in cases) == BY_CLASS

    # every case is a row of the table, under the row's switches, and files under the row's key
    rows = {tuple(r) for r in R.gold()["rows"]}
    for c in cases:
        row = (c.gi, c.B, c.wino, c.psplit) + c.plan
        assert row in rows, c.id
        assert R.key_of(row) == c.key and list(c.geom) == T.GEOMS[c.gi]
        assert c.psplit == 0 or c.gi == R.STEM

    # per key: the smallest batch of the group, and the largest not above MAX_B where that differs
    per_key = collections.defaultdict(list)
    for c in cases:
        per_key[c.key].append(c.B)
    for key, at in R.groups().items():
        small = min(at)
        big = max([b for b in at if b <= R.MAX_B] or [small])
        assert sorted(per_key[key]) == sorted({small, big}), key


def test_key_leaves_no_plan_column_out():
    """two rows with the same key differ in the batch, the statistics slice counts (the key has them
    per image) and the stem's override column alone"""
    free = {COL["batch"], COL["psplit"], COL["fwd_stats_slices"], COL["dgrad_stats_slices"]}
    first = {}
    for row in R.gold()["rows"]:
        key = R.key_of(row)
        if key is None:
            assert row[COL["class"]] == -1 or (row[COL["psplit"]] != 0 and row[COL["geom"]] != R.STEM)
            continue
        ref = first.setdefault(key, row)
        assert all(a == b for i, (a, b) in enumerate(zip(ref, row)) if i not in free), (ref, row)
    # the override does nothing for the geometries whose override rows are left out
    by_call = {tuple(r[:4]): r[4:] for r in R.gold()["rows"]}
    for (gi, B, wino, ps), plan in by_call.items():
        if gi != R.STEM:
            assert plan == by_call[(gi, B, wino, 0)]


def test_cases_cover_every_class_and_key_column_value():
    cases = R.cases()
    assert {c.cls for c in cases} == {0, 1, 2, 3, 4, 5}
    table_keys = [k for k in map(R.key_of, R.gold()["rows"]) if k is not None]
    for i, name in enumerate(R.KEY_COLUMNS):
        assert {c.key[i] for c in cases} == {k[i] for k in table_keys}, name
    # the batches that are no power of two, and the stem's smallest and largest slices
    assert {12, 24, 48, 96, 192, 384} <= {c.B for c in cases}
    assert {c.wgrad_imgs for c in cases if c.gi == R.STEM} == {1, 2, 4}
    assert {c.fwd_unit for c in cases if c.gi == R.STEM} == {1, 2, 4}
    # split-K factors that differ between the directions, and one Winograd direction alone
    assert {(4, 2), (2, 1), (1, 4), (1, 2)} <= {(c.fwd_ksplit, c.dgrad_ksplit) for c in cases}
    assert {(0, 1), (1, 0), (1, 1), (0, 0)} == {(c.fwd_wino, c.dgrad_wino) for c in cases}


def test_case_batches_tile():
    for c in R.cases():
        assert c.B % c.fwd_imgs == 0 and c.B % c.wgrad_imgs == 0, c.id
        assert c.fwd_stats_slices == 0 or (c.fwd_stats_slices % c.B == 0 if c.gi == R.STEM
                                           else c.B % c.fwd_stats_slices == 0), c.id
        assert c.dgrad_stats_slices == 0 or c.B % c.dgrad_stats_slices == 0, c.id
        assert c.B <= R.MAX_B or min(R.groups()[c.key]) > R.MAX_B, c.id


@pytest.mark.skipif(not native_available(), reason="extension not built")
def test_bindings_report_each_case_row():
    from network_distributed_pytorch_amd.ops import ext

    X = ext()
    bad = []
    try:
        for c in R.cases():
            X.wino_set_enabled(bool(c.wino))
            X.conv_set_stem_psplit(c.psplit)
            geom = list(c.geom)
            got = tuple(int(v) for v in X.conv_plan(geom, c.B)) + (
                int(X.conv_stats_slices(geom, c.B)), int(X.conv_dgrad_stats_slices(geom, c.B)),
                int(X.conv_wino(geom, c.B, False)), int(X.conv_wino(geom, c.B, True)))
            if got != c.plan:
                bad.append((c.id, got, c.plan))
    finally:
        X.wino_set_enabled(True)
        X.conv_set_stem_psplit(0)
    assert not bad, f"{len(bad)} cases differ (id, got, want), columns {R.PLAN_COLUMNS}: {bad[:5]}"
