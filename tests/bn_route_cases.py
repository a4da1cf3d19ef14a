"""The complete list of BatchNorm launch variants, one servable call each, from the recorded route
table tests/golden/bn_route_table.json alone (no extension, no GPU).

A variant key is (kind, training, mbeta, HW, route id): which binding is called (bn_fwd, bn_bwd,
bn_pair_fwd, bn_pair_bwd, the stem tail), in which mode, on which map size, and which row of the
table's `routes` the call is decided to (tools/bn_route_table.py COLUMNS: path, float4 or scalar
body, column-block width, row split, vector width, statistics pass or folded conv partials, slab
mode of either input, addend).  Refused calls (path "none") are no variant.

cases() gives one Case per key: over the float4-on rows of the table, among the shapes with
N >= MIN_N (no channel's statistics degenerate) the call with the smallest N * C * HW, the first in
grid order (tools/bn_route_table.py shapes(), then calls()) among equals.  Only calls that the
bindings serve count: the table asks bn_route about slabs on every shape, but the bindings take
slabs of whole float4 tensors only, so a call with slabs needs N * C * HW % 4 == 0 (servable()).
tests/test_bn_route_cases_cpu.py pins that no key is left out; tests/test_bn_routes_gpu.py runs
each Case against an fp64 reference after asserting that bn_route sends the tensors it built down
the Case's route.  switch_off_cases() adds the plain calls under bn_set_vec4(False), from the
table's float4-off rows.
"""
from __future__ import annotations

import functools
import json
import os
from typing import NamedTuple

from tools import bn_route_table as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bn_route_table.json")
MIN_N = 7
KINDS = ("bn_fwd", "bn_bwd", "pair_fwd", "pair_bwd", "stem_fwd")


class Case(NamedTuple):
    key: tuple      # (kind, training, mbeta, HW, route id)
    N: int
    C: int
    HW: int
    call: tuple     # CALL_COLUMNS
    route: tuple    # COLUMNS, the row gold["routes"][route id]
    shape: tuple    # SHAPE_COLUMNS of (HW, C, N): S, Sa, Ss, part_numel, blocks
    tag: str = ""   # "-v4off": a row of the table's float4-off part

    @property
    def kind(self):
        return self.key[0]

    @property
    def id(self):
        kind, training, mbeta, HW, rid = self.key
        return f"{kind}{'' if training else '-eval'}{'-mbeta' if mbeta else ''}-HW{HW}-r{rid}-N{self.N}C{self.C}{self.tag}"

    def __getattr__(self, name):  # a call or route column by name: case.nslab, case.path
        if name in T.CALL_COLUMNS:
            return self.call[T.CALL_COLUMNS.index(name)]
        if name in T.COLUMNS:
            return self.route[T.COLUMNS.index(name)]
        raise AttributeError(name)


def kind_of(call):
    bwd, pair, pool_w = (call[T.CALL_COLUMNS.index(c)] for c in ("bwd", "pair", "pool_w"))
    if pool_w:
        return "stem_fwd"
    return ("pair_bwd" if bwd else "pair_fwd") if pair else ("bn_bwd" if bwd else "bn_fwd")


def key_of(call, HW, rid):
    return (kind_of(call), bool(call[T.CALL_COLUMNS.index("training")]), bool(call[T.CALL_COLUMNS.index("mbeta")]),
            HW, rid)


@functools.lru_cache(maxsize=None)
def gold():
    with open(GOLDEN) as fh:
        g = json.load(fh)
    assert g["columns"] == T.COLUMNS and g["call_columns"] == T.CALL_COLUMNS
    assert g["shape_columns"] == T.SHAPE_COLUMNS + T.QUERY_COLUMNS + ["pattern"]
    assert g["axes"] == {"HW": T.HWS, "C": T.CS, "N": T.NS, "slabs": T.SLABS}
    return g


def table_calls(min_n=1):
    """(HW, C, N, shape row, call, route id) over the float4-on rows, in grid order"""
    g = gold()
    patterns = g["patterns"]
    for (HW, C, N), row in zip(T.shapes(), g["shapes"]):
        if N < min_n:
            continue
        *_front, pair_ok, pattern = row
        runs = patterns[pattern]
        rids = [rid for rid, n in zip(runs[0::2], runs[1::2]) for _ in range(n)]
        block = T.calls(HW, bool(pair_ok))
        assert len(rids) == len(block)
        for call, rid in zip(block, rids):
            yield HW, C, N, row, call, rid


def servable(call, numel):
    """the bindings take slabs of whole float4 tensors only (slab_input in csrc/bindings.cpp)"""
    nslab, nslab2 = call[T.CALL_COLUMNS.index("nslab")], call[T.CALL_COLUMNS.index("nslab2")]
    return (nslab < 2 and nslab2 < 2) or numel % 4 == 0


def all_keys():
    """every variant key of the table, whatever the batch size"""
    path = T.COLUMNS.index("path")
    routes = gold()["routes"]
    return {key_of(call, HW, rid) for HW, _C, _N, _row, call, rid in table_calls() if routes[rid][path] != 0}


@functools.lru_cache(maxsize=None)
def cases():
    path = T.COLUMNS.index("path")
    routes = gold()["routes"]
    best = {}
    for HW, C, N, row, call, rid in table_calls(MIN_N):
        if routes[rid][path] == 0 or not servable(call, N * C * HW):
            continue
        key = key_of(call, HW, rid)
        if key not in best or N * C * HW < best[key][0]:  # strict: the first in grid order stays
            best[key] = (N * C * HW, Case(key, N, C, HW, call, tuple(routes[rid]), tuple(row[:len(T.SHAPE_COLUMNS)])))
    order = {k: i for i, k in enumerate(KINDS)}
    return tuple(c for _, c in sorted(best.values(), key=lambda v: (order[v[1].key[0]], v[1].key[3], v[1].key[4],
                                                                    not v[1].key[1], v[1].key[2])))


# bn_set_vec4(False): one plain training forward and backward per single-launch map size
SWITCH_OFF_HWS = (1, 2, 4, 8, 16, 64)
SWITCH_OFF_NC = (7, 16)


def switch_off_cases(HW):
    """(forward Case, backward Case) at N = 7, C = 16 from the table's float4-off rows: all operands
    aligned, single launch allowed, no slabs, no external statistics"""
    g = gold()
    N, C = SWITCH_OFF_NC
    i = T.shapes().index((HW, C, N))
    row = dict(g["vec4_off"]).get(i, g["shapes"][i])
    runs = g["patterns"][row[-1]]
    rids = [rid for rid, n in zip(runs[0::2], runs[1::2]) for _ in range(n)]
    block = T.calls(HW, bool(row[-2]))
    out = []
    for bwd in (False, True):
        call = (bwd, True, True, False, 0, 0, 0, 0, True, False, False, (True, True, True, True))
        rid = rids[block.index(call)]
        out.append(Case(key_of(call, HW, rid), N, C, HW, call, tuple(g["routes"][rid]),
                        tuple(row[:len(T.SHAPE_COLUMNS)]), "-v4off"))
    return tuple(out)
