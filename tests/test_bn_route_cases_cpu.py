"""tests/bn_route_cases.py reaches every BatchNorm launch variant of the recorded route table: the
cases that tests/test_bn_routes_gpu.py runs against fp64 leave no variant key out.  Pure Python on
the fixture (no extension, no GPU).  If tests/golden/bn_route_table.json is regenerated and the
counts move, the numbers here move with it, in the same commit as the new fixture."""
import collections

from tests import bn_route_cases as R
from tools import bn_route_table as T

N_KEYS = 599
BY_PATH = {"fused": 414, "two-kernel": 138, "fused64": 32, "three-kernel": 15}
BY_KIND = {"bn_bwd": 200, "pair_fwd": 153, "bn_fwd": 141, "pair_bwd": 85, "stem_fwd": 20}
MAX_ELEMENTS = 528_384  # N = 129, C * HW = 4096


def test_cases_cover_every_variant_key():
    cases = R.cases()
    keys = [c.key for c in cases]
    assert len(cases) == N_KEYS and len(set(keys)) == N_KEYS
    assert set(keys) == R.all_keys()  # no key is exempt, whatever batch size reached it in the table
    assert len({c.id for c in cases}) == N_KEYS
    assert cases == R.cases() and [c.id for c in cases] == [c.id for c in R.cases.__wrapped__()]  # deterministic
    assert collections.Counter(T.PATHS[c.path] for c in cases) == BY_PATH
    assert collections.Counter(c.kind for c in cases) == BY_KIND

    routes = R.gold()["routes"]
    path = T.COLUMNS.index("path")
    assert {c.key[4] for c in cases} == {i for i, r in enumerate(routes) if r[path] != 0}
    assert all(c.route == tuple(routes[c.key[4]]) for c in cases)
    assert {c.HW for c in cases} == set(T.HWS)


def test_cases_are_small_servable_and_varied():
    cases = R.cases()
    assert all(c.N >= R.MIN_N for c in cases)
    assert max(c.N * c.C * c.HW for c in cases) <= MAX_ELEMENTS
    assert sum(c.N * c.C * c.HW for c in cases) < 32_000_000
    # the bindings refuse slabs of tensors that are no whole float4s
    assert all((c.nslab < 2 and c.nslab2 < 2) or (c.N * c.C * c.HW) % 4 == 0 for c in cases)
    # every alignment fact both ways, every slab count class on both inputs of the pair
    for k in range(4):
        assert {c.align[k] for c in cases} == {True, False}
    pair = [c for c in cases if c.kind == "pair_fwd"]
    assert {c.nslab for c in pair} == {c.nslab2 for c in pair} == {0, 2, 5}
    assert {(c.kind, c.ext_slices) for c in cases} >= {("bn_fwd", T.EXT), ("bn_bwd", T.EXT), ("stem_fwd", T.EXT)}
    assert any(c.mbeta for c in cases) and any(not c.training for c in cases) and any(c.addend for c in cases)


def test_switch_off_cases_come_from_the_float4_off_rows():
    col = {c: i for i, c in enumerate(T.COLUMNS)}
    for HW in R.SWITCH_OFF_HWS:
        fwd, bwd = R.switch_off_cases(HW)
        assert (fwd.kind, bwd.kind) == ("bn_fwd", "bn_bwd") and (fwd.N, fwd.C) == R.SWITCH_OFF_NC
        for c in (fwd, bwd):
            assert c.route[col["v4"]] == 0 and c.route[col["path"]] == (4 if HW == 64 else 1)
