"""The complete list of direct-conv plans, at most two servable batches each, from the recorded plan
table tests/golden/conv_plan_table.json alone (no extension, no GPU).

A plan key is (geometry index, Winograd switch, class, fwd_imgs, wgrad_imgs, dgrad_direct, fwd_ksplit,
dgrad_ksplit, forward partial unit, grad-x images per partial, fwd_wino, dgrad_wino): what
csrc/conv.hip conv_make_plan decides for a geometry, with the statistics slices counted per image
so that they do not split a group by batch alone.  The forward partial unit is B // fwd_stats_slices
(0: no forward partials); for the stem it is fwd_stats_slices // B, the output-row blocks per image,
which folds the conv_set_stem_psplit override column of the table into the key.  The grad-x unit is
B // dgrad_stats_slices (0: none).  Rows of other geometries count at psplit == 0 only (the override
does nothing for them), class -1 rows are no key, and the Winograd switch stays in the key where both
values give the same plan columns: launch_conv_wgrad chooses the layer1 Winograd grad-W from the
switch, not from the plan.

cases() gives each key the smallest batch of its group and, when that differs, the largest batch of
its group that is not above MAX_B.  The second reaches the batches that are no power of two and the
kernel choices that depend on the batch without showing in the plan (the 2-wave Winograd grad-W
reduction from batch 512, kConv3x3S2 pairing only up to 256).  A group whose only batches are above
MAX_B keeps its smallest.  tests/test_conv_plan_cases_cpu.py pins that no key is left out;
tests/test_conv_plans_gpu.py runs each Case against an fp64 reference after asserting that the
bindings report the Case's plan row.
"""
from __future__ import annotations

import functools
import json
import os
from typing import NamedTuple

from tools import conv_plan_table as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan_table.json")
MAX_B = 512
STEM = T.GEOMS.index([3, 32, 32, 64, 7, 7, 2, 3])
KEY_COLUMNS = ["geom", "wino", "class", "fwd_imgs", "wgrad_imgs", "dgrad_direct", "fwd_ksplit", "dgrad_ksplit",
               "fwd_unit", "dgrad_unit", "fwd_wino", "dgrad_wino"]
_COL = {c: i for i, c in enumerate(T.COLUMNS)}
PLAN_COLUMNS = T.COLUMNS[_COL["class"]:]  # what the four bindings report for (geometry, batch)


class Case(NamedTuple):
    key: tuple    # KEY_COLUMNS
    gi: int       # index into tools/conv_plan_table.py GEOMS
    geom: tuple   # (C, H, W, Co, KH, KW, stride, pad)
    B: int
    wino: int     # wino_set_enabled
    psplit: int   # conv_set_stem_psplit (0 but for the stem's override rows)
    plan: tuple   # PLAN_COLUMNS of the table's row

    @property
    def id(self):
        C, H, W, Co, KH, KW, s, _p = self.geom
        rb = f"-rb{self.key[KEY_COLUMNS.index('fwd_unit')]}" if self.gi == STEM else ""
        return (f"g{self.gi}-{C}x{H}x{W}-{Co}-{KH}x{KW}s{s}-B{self.B}-{'wino' if self.wino else 'direct'}"
                f"-ks{self.fwd_ksplit}.{self.dgrad_ksplit}-wg{self.wgrad_imgs}{rb}")

    def __getattr__(self, name):  # a plan or key column by name: case.fwd_ksplit, case.fwd_unit; "class" is case.cls
        name = "class" if name == "cls" else name
        if name in PLAN_COLUMNS:
            return self.plan[PLAN_COLUMNS.index(name)]
        if name in KEY_COLUMNS:
            return self.key[KEY_COLUMNS.index(name)]
        raise AttributeError(name)


@functools.lru_cache(maxsize=None)
def gold():
    with open(GOLDEN) as fh:
        g = json.load(fh)
    assert g["columns"] == T.COLUMNS and g["geoms"] == T.GEOMS
    return g


def key_of(row):
    """the plan key of a table row, or None where the row is no key"""
    r = dict(zip(T.COLUMNS, row))
    if r["class"] < 0 or (r["geom"] != STEM and r["psplit"] != 0):
        return None
    B, fs, ds = r["batch"], r["fwd_stats_slices"], r["dgrad_stats_slices"]
    fwd_unit = 0 if fs == 0 else (fs // B if r["geom"] == STEM else B // fs)
    return (r["geom"], r["wino"], r["class"], r["fwd_imgs"], r["wgrad_imgs"], r["dgrad_direct"], r["fwd_ksplit"],
            r["dgrad_ksplit"], fwd_unit, 0 if ds == 0 else B // ds, r["fwd_wino"], r["dgrad_wino"])


@functools.lru_cache(maxsize=None)
def groups():
    """key -> {batch: row}; at a batch that several rows of the stem reach, the row without override"""
    out: dict = {}
    for row in gold()["rows"]:
        key = key_of(row)
        if key is None:
            continue
        at = out.setdefault(key, {})
        B = row[_COL["batch"]]
        if B not in at or row[_COL["psplit"]] < at[B][_COL["psplit"]]:
            at[B] = row
    return out


def all_keys():
    return set(groups())


def _case(key, row):
    r = dict(zip(T.COLUMNS, row))
    return Case(key, r["geom"], tuple(T.GEOMS[r["geom"]]), r["batch"], r["wino"], r["psplit"],
                tuple(row[_COL["class"]:]))


@functools.lru_cache(maxsize=None)
def cases():
    """sorted by (geometry, batch, switch, key), so that the cases which share a reference are neighbours"""
    out = []
    for key, at in groups().items():
        small = min(at)
        big = max((b for b in at if b <= MAX_B), default=small)
        out += [_case(key, at[b]) for b in ([small] if big == small else [small, big])]
    return tuple(sorted(out, key=lambda c: (c.gi, c.B, -c.wino, c.key)))
