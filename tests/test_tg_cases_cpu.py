"""tests/tg_cases.py reaches every tgemm kernel instance and launch-shape edge of csrc/tgemm.hip: the
coverage is asserted from the literals each case claims, so that a bullet fails when it loses its last
case; with the extension built, tg_describe -- which shares its load-width and slab decision with
run() -- reports the same facts for every case, and the set of (direction, instance) pairs it
gives over a stated grid of geometries, batches and operand misalignments equals the table's.
Host code only."""
import itertools

import pytest

from network_distributed_pytorch_amd.ops import native_available
from tests import tg_cases as T

needs_ext = pytest.mark.skipif(not native_available(), reason="extension not built")

N_CASES = 63


def _cases(d, pred=lambda c: True):
    return [c for c in T.CASES if c.dir == d and pred(c)]


def test_case_list_is_well_formed():
    assert len(T.CASES) == N_CASES and len({c.name for c in T.CASES}) == N_CASES
    for c in T.CASES:
        B, C, H, W, Co = c.shape
        hw = H * W
        assert c.name.startswith(T.DIR_NAMES[c.dir] + "-"), c.name
        assert hw >= 2 and hw & (hw - 1) == 0, c.name
        assert all(n % 4 == 0 and n <= T.MAX_ELEMS for n in c.sizes()), c.name   # what tg_plan accepts
        assert c.a_off in (0, 4) and c.b_off in (0, 4), c.name
        assert not c.addend or c.dir == T.DGRAD, c.name
        assert not (c.addend and c.defer), c.name        # an addend is never deferred
        assert not c.defer or c.slabs > 1, c.name        # a deferred case leaves slabs
        # the claimed facts agree with each other
        assert (c.M, c.N, c.K) == {T.FWD: (Co, B * hw, C), T.DGRAD: (C, B * hw, Co), T.WGRAD: (Co, C, B * hw)}[c.dir]
        assert c.slabs == -(-c.ktiles // c.per) and 1 <= c.slabs <= c.splits, c.name
        assert (c.slabs - 1) * c.kchunk < c.K <= c.slabs * c.kchunk, c.name
        assert 9 * c.K <= 9504, c.name                   # integer operands in [-3, 3] stay exact in fp32
        assert c.pair in T.PAIRS, c.name


def test_every_instance_has_a_case():
    assert {c.pair for c in T.CASES} == T.PAIRS
    assert len(T.PAIRS) == 17 and len({i for _, i in T.PAIRS}) == 14


def test_every_instance_runs_more_than_one_k_tile():
    """past the prologue: a second k-tile reaches the LDS stores inside the k loop and the other LDS
    buffer, for the scalar (W = 1) and 2-pixel (BNF / AKF false) mappings too"""
    for pair in T.PAIRS:
        assert any(c.pair == pair and c.per >= 2 for c in T.CASES), pair


@pytest.mark.parametrize("d", (T.FWD, T.DGRAD, T.WGRAD))
def test_k_loop_phases_and_tile_edges(d):
    cs = _cases(d)
    assert {c.per for c in cs} >= set(T.PER_SPLIT[d])
    assert any(c.K % T.BK != 0 and c.K > T.BK for c in cs)
    assert any(c.K < T.BK for c in cs)
    for dim in ("M", "N"):
        v = [getattr(c, dim) for c in cs]
        assert any(x < 32 for x in v), dim
        assert any(32 < x < 64 for x in v), dim
        assert any(x == 64 for x in v), dim
        assert any(x > 64 for x in v), dim


@pytest.mark.parametrize("d", (T.FWD, T.DGRAD))
def test_forward_and_grad_x_splits(d):
    assert {c.slabs for c in _cases(d)} >= {1, 2, 4}
    assert {c.splits for c in _cases(d)} >= {1, 2, 4}
    # fewer slabs launched than allotted, and a last split that is shorter and ends inside a k-tile
    assert _cases(d, lambda c: c.slabs < c.splits)
    assert _cases(d, lambda c: c.slabs > 1 and c.K % c.kchunk != 0 and c.K % T.BK != 0)


def test_grad_w_splits():
    k1056, k1044 = T.by_name("wgrad-k1056"), T.by_name("wgrad-k1044")
    assert k1056.shape == (66, 64, 4, 4, 64) and k1056.K == 1056 and k1056.ktiles == 33
    assert 1 < k1056.slabs < k1056.splits
    assert k1044.K == 1044 and 1 < k1044.slabs < k1044.splits
    last = k1044.K - (k1044.slabs - 1) * k1044.kchunk
    assert 0 < last < k1044.kchunk and last % T.BK != 0
    assert _cases(T.WGRAD, lambda c: c.slabs == c.splits == 2)


def test_defer_and_addend_variants():
    for d in (T.FWD, T.DGRAD, T.WGRAD):
        assert _cases(d, lambda c: c.defer and c.slabs > 1), d
        assert _cases(d, lambda c: c.defer and c.slabs < c.splits), d   # scratch slabs past the count stay
    add = _cases(T.DGRAD, lambda c: c.addend)
    # in place in the epilogue: M ragged inside one tile and inside the second (the clamped address)
    assert any(c.slabs == 1 and c.M < 64 and c.M % 32 != 0 for c in add)
    assert any(c.slabs == 1 and c.M > 64 and c.M % 64 != 0 for c in add)
    assert any(c.slabs == 1 and c.instance.endswith("11") for c in add)
    # through the slab sum
    assert any(c.slabs > 1 for c in add) and any(1 < c.slabs < c.splits for c in add)


@needs_ext
@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_describe_reports_the_claimed_facts(case):
    from network_distributed_pytorch_amd.ops import ext

    assert ext().tg_plan(case.geom, case.B)[0] == 0
    assert ext().tg_plan(case.geom, case.B)[1 + case.dir] == case.splits
    d = ext().tg_describe(case.geom, case.B, case.dir, case.a_off, case.b_off)
    assert T.instance_name(d) == case.instance
    assert (d["M"], d["N"], d["K"]) == (case.M, case.N, case.K)
    assert (d["splits"], d["slabs"], d["kchunk"]) == (case.splits, case.slabs, case.kchunk)
    # the defaults are aligned operands
    assert ext().tg_describe(case.geom, case.B, case.dir) == ext().tg_describe(case.geom, case.B, case.dir, 0, 0)


@needs_ext
def test_table_covers_every_reachable_instance():
    """tg_describe over channels x maps x batches x directions x misalignments, at the geometries
    tg_plan accepts: the (direction, AKF, BNF, wa, wb) that occur are exactly the table's"""
    from network_distributed_pytorch_amd.ops import ext

    seen, swept = set(), 0
    for C, Co, (H, W), B in itertools.product(T.SWEEP_CHANNELS, T.SWEEP_CHANNELS, T.SWEEP_MAPS, T.SWEEP_BATCHES):
        geom = [C, H, W, Co, 1, 1, 1, 0]
        if ext().tg_plan(geom, B)[0] < 0:
            continue
        swept += 1
        for d in (T.FWD, T.DGRAD, T.WGRAD):
            for a_off, b_off in T.SWEEP_OFFS:
                r = ext().tg_describe(geom, B, d, a_off, b_off)
                assert r["wa"] in (1, 4) and r["wb"] in (1, 4) and 1 <= r["slabs"] <= r["splits"]
                seen.add((d, r["akf"], r["bnf"], r["wa"], r["wb"]))
    assert swept == 8 * 8 * 5 * 4   # even channels and batches: tg_plan accepts the whole grid
    table = {(c.dir, c.instance[0] == "T", c.instance[1] == "T", int(c.instance[2]), int(c.instance[3]))
             for c in T.CASES}
    assert seen == table, (sorted(seen - table), sorted(table - seen))


@needs_ext
def test_describe_rejects_bad_arguments():
    from network_distributed_pytorch_amd.ops import ext

    geom = [8, 2, 2, 4, 1, 1, 1, 0]
    for bad in ((3, 0, 0), (0, 16, 0), (0, 0, -4)):
        with pytest.raises(RuntimeError):
            ext().tg_describe(geom, 2, *bad)
