"""The BatchNorm launch route as the bindings report it (csrc/batchnorm.hip bn_make_route through
bn_route), over a grid of shapes, call kinds, slab counts, external statistics, alignment facts and
the float4 switch.

    python tools/bn_route_table.py --legacy-only > legacy.json          (any build, also one
                                                                          from before bn_route)
    python tools/bn_route_table.py --legacy legacy.json > tests/golden/bn_route_table.json

writes the fixture that tests/test_bn_route_cpu.py compares a build against (host code only, no
GPU).  --legacy refuses to write a table whose bn_two_kernel_path, bn_pair_ok, bn_slices and
bn_part_numel answers differ from the recorded ones: that is how the fixture was tied to the build
from before the route existed.  Regenerate it only from a build whose launches are known good.

The grid is large (about a million calls), so the table is stored in three levels.  `shapes` has one
row per (HW, C, N) under float4 on: what follows from the shape alone (SHAPE_COLUMNS; S and
part_numel are also what bn_slices and bn_part_numel answer), the shape-only queries
(QUERY_COLUMNS) and the shape's pattern.  `vec4_off` lists (shape index, row) where float4 off
changes a row.  `routes` lists every distinct remainder of a route once (COLUMNS; grid = blocks *
split).  `patterns` lists every distinct run-length-coded sequence (route id, count, ...) over the
calls of one shape, in calls() order.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

HWS = [1, 2, 4, 6, 8, 16, 49, 64, 256, 1024]
CS = [5, 16, 64, 128, 256, 512, 1024, 2048]
NS = [1, 3, 7, 8, 15, 16, 17, 64, 100, 127, 128, 129, 256, 512, 513, 8192]
SLABS = [0, 1, 2, 4, 5, 8]
VEC4 = [1, 0]            # bn_set_vec4
EXT = 7                  # partials per channel of offered external statistics
POOL_W = {4: 2, 16: 4, 64: 8, 256: 16, 1024: 32}  # stem-tail rows: square maps

PATHS = {0: "none", 1: "fused", 2: "fused64", 3: "three-kernel", 4: "two-kernel"}
SLAB = {0: "none", 1: "in-kernel", 2: "sum-first"}
# bn_route returns these, in this order
ROUTE_COLUMNS = ["path", "v4", "CW", "MAXN", "split", "grid", "vec", "S", "Sa", "stats_pass", "Sp", "Ss", "slab",
                 "slab2", "addend", "part_numel"]
# per shape: these route values, then blocks = grid / split of its single-launch routes (0: it has none)
SHAPE_COLUMNS = ["S", "Sa", "Ss", "part_numel", "blocks"]
QUERY_COLUMNS = ["two_kernel_path(single=0)", "two_kernel_path(single=1)", "pair_ok"]
COLUMNS = [c for c in ROUTE_COLUMNS if c not in SHAPE_COLUMNS and c != "grid"]
# a call: bn_route's arguments after the shape
CALL_COLUMNS = ["bwd", "training", "single", "pair", "pool_w", "nslab", "nslab2", "ext_slices", "relu", "addend",
                "mbeta", "align"]
_SHAPE_IDX = [ROUTE_COLUMNS.index(c) for c in SHAPE_COLUMNS[:-1]]
_GRID, _SPLIT = ROUTE_COLUMNS.index("grid"), ROUTE_COLUMNS.index("split")
_REST_IDX = [ROUTE_COLUMNS.index(c) for c in COLUMNS]


def _aligns(fused, two, slabs, slabs2):
    """every alignment bool that the call has, both ways; the others stay true"""
    return [(f, t, s, s2) for f in ((True, False) if fused else (True,)) for t in ((True, False) if two else (True,))
            for s in ((True, False) if slabs else (True,)) for s2 in ((True, False) if slabs2 else (True,))]


def calls(HW, pair_ok):
    """The calls the bindings accept for one shape, as bn_route argument tuples (CALL_COLUMNS)."""
    out = []
    for single in (False, True):
        # bn_fwd: slabs need training mode, external statistics need training and no slabs
        for training in (True, False):
            for ns in SLABS if training else SLABS[:2]:
                for ext in ((0, EXT) if training and ns < 2 else (0,)):
                    for al in _aligns(True, True, ns >= 2, False):
                        out.append((False, training, single, False, 0, ns, 0, ext, True, False, False, al))
        # bn_bwd: external statistics come without a slab tensor, the addend only with one
        for ns in SLABS:
            for ext in ((0, EXT) if ns == 0 else (0,)):
                for addend in ((False, True) if ns >= 2 else (False,)):
                    for al in _aligns(True, True, ns >= 2, False):
                        out.append((True, True, single, False, 0, ns, 0, ext, True, addend, False, al))
        # bn_bwd with the mask recomputed from x (no y, no slabs); rejected rows are path "none"
        for al in _aligns(False, True, False, False):
            out.append((True, True, single, False, 0, 0, 0, 0, True, False, True, al))
    if pair_ok:  # bn_pair_fwd / bn_pair_bwd reject every other shape
        for ns in SLABS:
            for ns2 in SLABS:
                for al in _aligns(True, False, ns >= 2, ns2 >= 2):
                    out.append((False, True, True, True, 0, ns, ns2, 0, True, False, False, al))
            for addend in ((False, True) if ns >= 2 else (False,)):
                for al in _aligns(True, False, ns >= 2, False):
                    out.append((True, True, True, True, 0, ns, 0, 0, True, addend, False, al))
    if HW in POOL_W:  # bn_relu_maxpool
        for ext in (0, EXT):
            for al in _aligns(False, True, False, False):
                out.append((False, True, False, False, POOL_W[HW], 0, 0, ext, True, False, False, al))
    return out


def shapes():
    return [(HW, C, N) for HW in HWS for C in CS for N in NS]


def legacy_rows(X):
    """[two_kernel_path(single=0), (single=1), pair_ok, slices, part_numel] per (shape, vec4) in
    shapes() x VEC4 order; leaves bn_set_vec4 on."""
    out = []
    try:
        for HW, C, N in shapes():
            for v in VEC4:
                X.bn_set_vec4(bool(v))
                out.append([int(X.bn_two_kernel_path(N, C, HW, False)), int(X.bn_two_kernel_path(N, C, HW, True)),
                            int(X.bn_pair_ok(N, C, HW)), int(X.bn_slices(N, C, HW)), int(X.bn_part_numel(N, C, HW))])
    finally:
        X.bn_set_vec4(True)
    return out


def table(X, legacy=None):
    """The whole fixture as a dict; leaves bn_set_vec4 on."""
    mine = legacy_rows(X)
    assert legacy is None or legacy == mine, "the shape-only queries differ from the recorded ones"
    rows = {1: [], 0: []}
    routes, route_id, patterns, pattern_id = [], {}, [], {}
    try:
        for i, (HW, C, N) in enumerate(shapes()):
            for j, v in enumerate(VEC4):
                X.bn_set_vec4(bool(v))
                two0, two1, pair_ok, slices, part_numel = mine[i * len(VEC4) + j]
                runs, shape, blocks = [], None, 0
                for c in calls(HW, bool(pair_ok)):
                    r = [int(t) for t in X.bn_route(c[0], N, C, HW, *c[1:])]
                    s = [r[k] for k in _SHAPE_IDX]
                    assert shape in (None, s), "a shape column varies inside one shape"
                    shape = s
                    if r[_GRID]:
                        assert r[_GRID] % r[_SPLIT] == 0 and blocks in (0, r[_GRID] // r[_SPLIT])
                        blocks = r[_GRID] // r[_SPLIT]
                    rest = tuple(r[k] for k in _REST_IDX)
                    rid = route_id.setdefault(rest, len(routes))
                    if rid == len(routes):
                        routes.append(list(rest))
                    if runs and runs[-2] == rid:
                        runs[-1] += 1
                    else:
                        runs += [rid, 1]
                assert (shape[0], shape[3]) == (slices, part_numel), "bn_slices / bn_part_numel differ from the route"
                pid = pattern_id.setdefault(tuple(runs), len(patterns))
                if pid == len(patterns):
                    patterns.append(runs)
                rows[v].append(shape + [blocks, two0, two1, pair_ok, pid])
    finally:
        X.bn_set_vec4(True)
    return {"columns": COLUMNS, "shape_columns": SHAPE_COLUMNS + QUERY_COLUMNS + ["pattern"],
            "call_columns": CALL_COLUMNS, "axes": {"HW": HWS, "C": CS, "N": NS, "slabs": SLABS},
            "shapes": rows[1], "vec4_off": [[i, r] for i, (r, q) in enumerate(zip(rows[0], rows[1])) if r != q],
            "routes": routes, "patterns": patterns}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legacy-only", action="store_true", help="print the shape-only queries' answers alone")
    ap.add_argument("--legacy", help="answers recorded with --legacy-only that this build must reproduce")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from network_distributed_pytorch_amd.ops import ext

    def dumps(v):
        return json.dumps(v, separators=(",", ":"))

    def lines(rows, per=1):
        return "[\n" + ",\n".join(",".join(dumps(r) for r in rows[k:k + per]) for k in range(0, len(rows), per)) + "\n]"

    if args.legacy_only:
        print(lines(legacy_rows(ext())))
        return
    legacy = None
    if args.legacy:
        with open(args.legacy) as fh:
            legacy = json.load(fh)
    t = table(ext(), legacy)
    head = ",\n".join('"%s":%s' % (k, json.dumps(t[k])) for k in ("columns", "shape_columns", "call_columns", "axes"))
    body = ",\n".join('"%s":%s' % (k, lines(t[k], per)) for k, per in (("shapes", len(NS)), ("vec4_off", len(NS)),
                                                                         ("routes", 8), ("patterns", 1)))
    print("{%s,\n%s}" % (head, body))


if __name__ == "__main__":
    main()
