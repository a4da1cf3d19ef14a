"""The BatchNorm launch route (csrc/batchnorm.hip bn_make_route, read through the bn_route binding)
against the recorded table tests/golden/bn_route_table.json: every path, column-block width, row
split, vector width and slab outcome over shapes x call kinds x slab counts x external statistics
x alignment facts x the float4 switch.  Host code only.  tools/bn_route_table.py wrote the table
from the first build with the route, after its launches had been compared on the GPU with those of
the build before it, and only because bn_two_kernel_path, bn_pair_ok, bn_slices and bn_part_numel
answered as that earlier build (which combined its path predicates by hand) had been recorded to."""
import json
import os

import pytest

from network_distributed_pytorch_amd.ops import native_available

pytestmark = pytest.mark.skipif(not native_available(), reason="extension not built")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bn_route_table.json")


def test_bn_route_table():
    from network_distributed_pytorch_amd.ops import ext
    from tools import bn_route_table as T

    with open(GOLDEN) as fh:
        gold = json.load(fh)
    assert gold["columns"] == T.COLUMNS and gold["call_columns"] == T.CALL_COLUMNS
    assert gold["shape_columns"] == T.SHAPE_COLUMNS + T.QUERY_COLUMNS + ["pattern"]
    assert gold["axes"] == {"HW": T.HWS, "C": T.CS, "N": T.NS, "slabs": T.SLABS}
    shapes = T.shapes()
    assert len(gold["shapes"]) == len(shapes)

    # the fixture holds every decision the route can make
    col = {c: i for i, c in enumerate(T.COLUMNS)}
    routes, patterns = gold["routes"], gold["patterns"]
    off = dict(gold["vec4_off"])
    rows = [(sh, v, off.get(i, r) if not v else r) for i, (sh, r) in enumerate(zip(shapes, gold["shapes"])) for v in (1, 0)]
    assert {r[-1] for _, _, r in rows} == set(range(len(patterns)))
    assert {rid for p in patterns for rid in p[0::2]} == set(range(len(routes)))
    assert {r[col["path"]] for r in routes} == set(T.PATHS)
    fused = [r for r in routes if r[col["path"]] in (1, 2)]
    assert {r[col["CW"]] for r in fused} == {4, 8, 16, 64}
    assert {r[col["split"]] for r in fused} == {1, 2, 4}
    assert {r[col["v4"]] for r in fused} == {0, 1}
    assert {r[col["vec"]] for r in routes if r[col["path"]] == 4} == {0, 1}
    assert {r[col["slab"]] for r in routes} == set(T.SLAB) == {r[col["slab2"]] for r in routes}
    assert {(r[col["slab"]], r[col["addend"]]) for r in routes} >= {(1, 1), (2, 1), (1, 0), (2, 0)}

    X = ext()
    got = T.table(X)  # restores the switch in a finally; asserts bn_slices / bn_part_numel == the route's
    for key in ("shapes", "vec4_off", "routes", "patterns"):
        bad = [(i, g, w) for i, (g, w) in enumerate(zip(got[key], gold[key])) if g != w]
        assert len(got[key]) == len(gold[key]) and not bad, f"{key}: {len(bad)} entries differ (index, got, want): {bad[:3]}"

    # the shape-only queries say what the route says, in every row
    calls = 0
    for (HW, C, N), v, (*_shape, two0, two1, pair_ok, pattern) in rows:
        runs = patterns[pattern]
        paths = [routes[rid][col["path"]] for rid, n in zip(runs[0::2], runs[1::2]) for _ in range(n)]
        block = T.calls(HW, bool(pair_ok))
        assert len(paths) == len(block)
        calls += len(block)
        for (bwd, training, single, pair, pool_w, *_rest, mbeta, _al), path in zip(block, paths):
            if pair:
                assert path == 1
            elif pool_w or not (bwd or training):
                assert path == 4  # the stem tail and evaluation mode: always the two-kernel path
            elif mbeta:
                assert path == (4 if (two0, two1)[single] and HW % 4 == 0 else 0)
            else:
                assert (path == 4) == bool((two0, two1)[single]), (HW, C, N, v, single)
        if not pair_ok:  # and a pair outside bn_pair_ok is refused
            X.bn_set_vec4(bool(v))
            try:
                assert X.bn_route(False, N, C, HW, pair=True, single=True)[0] == 0
            finally:
                X.bn_set_vec4(True)
    assert calls > 900_000
