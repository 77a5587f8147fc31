"""The equality prefilter (csrc/pa_eq_any.h), the nt column stream and the one-launch reset of the lane-major scan
(scan_kernel's hoisted single-range loop), against the oracle.

A small table only reaches the hoisted loop when a wave owns several tiles of a segment, hence tuning scan_grid = 2 (two
workgroups of four waves) over segments of 64 whole wave tiles (2048 docs each) and a ragged one of 77 docs. The filter
column f holds nb-bit dictIds for every nb in 1..31: the forward index is packed nb bits wide, the dictionary holds
min(2^nb, 2^20) values (the C-ABI takes the width per column, and a 2^30-entry dictionary would not fit a test). The
value looked for sits only where it is planted: docs 0, 31, 32 and 2047 (first and last doc of a lane, first and last
lane of a tile), 2048 (the next tile), a run of adjacent docs inside one tile (crossing a lane), and a doc of the ragged
tail; every other doc holds another dictId, among them the neighbours v - 1, v + 1 and v with one bit flipped.

Every width runs the direct lane-major kernel: below 12 bits the planner expects a dense result and would take the
dense GROUP BY kernel, so those cases set PA_QF_NO_DENSE_GROUP. By default the prefilter is on only next to the nt
stream, which a table this small does not get, so the cases turn it on with tuning eq_prefilter = 1 (and once through
auto with stream_nt = 1).

Bars: bit-exact group keys, LONG SUMs and numDocsScanned; plans as reported by stats()["plan"].
"""
import numpy as np
import pytest
import torch

import oracle
from pinot_amd import _lib as L
from pinot_amd import parse_sql
from pinot_amd.engine import GpuQueryExecutor, GpuSegment
from pinot_amd.segment import pack_bits, segment_from_dict_ids
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

TILE = 2048
DOCS = 64 * TILE + 77
GRID = {"scan_grid": 2}
EQ_MAX_NB = 24  # kEqPrefilterMaxNb (csrc/pa_device.h): the widest column the prefilter takes
RUN_AT = 5 * TILE + 29  # a run of 6 adjacent matches: docs 29..34 of tile 5, i.e. lanes 0 and 1
PLANTED = (0, 31, 32, 2047, 2048) + tuple(range(RUN_AT, RUN_AT + 6)) + (64 * TILE + 50,)


def _segment(nb, seed, planted=PLANTED, target=None, base=0):
    """(segment, value of f looked for). f: dictionary base + 3 * arange(card), card = min(2^nb, 2^20); the target
    dictId defaults to a high one (all-ones in the low bits for a full-width dictionary)."""
    rng = np.random.default_rng(seed)
    card = min(1 << nb, 1 << 20)
    fdict = base + 3 * np.arange(card, dtype=np.int64)
    t = (card - 1 if seed % 2 else card // 3) if target is None else target
    if card == 1:
        raise ValueError("nb >= 1 means at least two values")
    ids = rng.integers(0, card - 1, size=DOCS, dtype=np.int64)
    ids[ids >= t] += 1  # uniform over the other dictIds
    near = [v for v in (t - 1, t + 1, t ^ 1, t ^ (1 << (max(nb, 1) - 1)), t ^ (1 << (nb // 2))) if 0 <= v < card and v != t]
    if near:
        where = rng.choice(DOCS, size=4000, replace=False)
        ids[where] = rng.choice(near, size=len(where))
    for d in planted:
        ids[d] = t
    g = rng.integers(0, 8, size=DOCS, dtype=np.int64)
    s = rng.integers(0, 1000, size=DOCS, dtype=np.int64)
    specs = {
        "f": ("INT", fdict, np.zeros((DOCS * nb + 7) // 8, dtype=np.uint8)),
        "g": ("INT", np.arange(8, dtype=np.int64) * 10, pack_bits(g.astype(np.uint32), 3)),
        "s": ("LONG", np.arange(1000, dtype=np.int64) * 1_000_003, pack_bits(s.astype(np.uint32), 10)),
    }
    seg = segment_from_dict_ids("eq%d_%d" % (nb, seed), DOCS, specs)
    f = seg.column("f")
    f.num_bits = nb  # (wider than the dictionary needs once nb > 20)
    f.fwd_bytes = pack_bits(ids.astype(np.uint32), nb)
    return seg, int(fdict[t])


def _sql(value, where=None):
    return "SELECT g, SUM(s) FROM t WHERE %s GROUP BY g LIMIT 100" % (where or "f IN (%d)" % value)


ON = {"eq_prefilter": 1}  # (auto turns the prefilter on only next to the nt stream, which these small tables do not get)


def _run(sql, gsegs, tuning=None, execution_stats=False, flags=0):
    q = parse_sql(sql)
    ex = GpuQueryExecutor(q, gsegs, flags=flags, tuning=dict(GRID, **(tuning or {})))
    try:
        plan = ex.stats()["plan"]
        ex.execute()
        got = ex.fetch(execution_stats=execution_stats)
    finally:
        ex.close()
    return q, plan, got


def _direct(plan):
    """The plan runs scan_kernel's lane-major variant (where the prefilter lives), not a dense or partitioned kernel."""
    return plan["lane_major"] == 1 and plan["strategy"] in ("lds", "global", "lane")


@pytest.fixture(scope="module")
def seg17():
    seg, v = _segment(17, 2)
    g = GpuSegment(seg)
    yield seg, g, v
    g.close()


@pytest.mark.parametrize("nb", range(1, 32))
def test_equality_of_every_width(nb):
    """Every width runs the direct lane-major plan with one eager literal: from 12 bits up the planner chooses it (one
    doc in 4096 or fewer matches: sparse), below that its estimate is a dense result and PA_QF_NO_DENSE_GROUP keeps the
    direct kernel. Prefilter on, off, and auto next to a forced nt stream give the oracle's result; on and auto + nt
    report the prefilter up to EQ_MAX_NB bits, auto alone never does here."""
    seg, v = _segment(nb, nb)
    flags = L.PA_QF_NO_DENSE_GROUP if nb < 12 else 0
    g = GpuSegment(seg)
    try:
        q, plan, got = _run(_sql(v), [g], ON, flags=flags)
        _, plan0, got0 = _run(_sql(v), [g], {"eq_prefilter": 0}, flags=flags)
        _, plan_nt, got_nt = _run(_sql(v), [g], {"stream_nt": 1}, flags=flags)
        _, plan_auto, _ = _run(_sql(v), [g], flags=flags)
    finally:
        g.close()
    print("nb=%d plan=%s" % (nb, plan))
    exp = oracle.run_query(q, [seg])
    assert exp.num_docs_scanned >= len(PLANTED)
    assert_same(got, exp)
    assert_same(got0, exp)
    assert_same(got_nt, exp)
    for p in (plan, plan0, plan_nt, plan_auto):
        assert _direct(p) and p["lane_major"] == 1 and p["eager_literals"] == 1, p
    want = 1 if nb <= EQ_MAX_NB else 0
    assert plan["eq_prefilter"] == want, plan
    assert plan_nt["eq_prefilter"] == want and plan_nt["stream_nt"] == 1, plan_nt
    assert plan0["eq_prefilter"] == 0 and plan_auto["eq_prefilter"] == 0, (plan0, plan_auto)


def test_absent_value_and_no_match(seg17):
    """A value the dictionary lacks, and a value of the dictionary that no doc holds: no docs, no groups."""
    seg, g, v = seg17
    q, plan, got = _run(_sql(v + 1), [g])  # (the dictionary's values are multiples of 3 apart)
    assert_same(got, oracle.run_query(q, [seg]))
    assert got.num_docs_scanned == 0 and not got.groups
    seg2, v2 = _segment(17, 3, planted=())
    g2 = GpuSegment(seg2)
    try:
        q2, plan2, got2 = _run(_sql(v2), [g2], ON)
    finally:
        g2.close()
    assert plan2["eq_prefilter"] == 1, plan2
    assert got2.num_docs_scanned == 0 and not got2.groups
    assert_same(got2, oracle.run_query(q2, [seg2]))


def test_two_segments_with_their_own_dictionaries():
    """The value has another dictId, in a column of another width, in each segment: the pattern changes at the segment
    switch (a wave's tiles span both segments at scan_grid = 2)."""
    a, va = _segment(17, 5, target=2001, base=0)
    b, vb = _segment(13, 6, target=(va - 300) // 3, base=300)
    assert va == vb  # dictId 2001 of 17 bits in the first segment, 1901 of 13 bits in the second
    gs = [GpuSegment(a), GpuSegment(b)]
    try:
        q, plan, got = _run(_sql(va), gs, ON)
        _, plan0, got0 = _run(_sql(va), gs, {"eq_prefilter": 0})
    finally:
        for g in gs:
            g.close()
    exp = oracle.run_query(q, [a, b])
    assert plan["eq_prefilter"] == 1 and plan["lane_major"] == 1 and plan["eager_literals"] == 1, plan
    assert exp.num_docs_scanned == 2 * len(PLANTED)
    assert_same(got, exp)
    assert_same(got0, exp)


def test_negated_and_two_leaf_filters_keep_their_paths(seg17):
    """NOT EQUALS, and ORs of two literals (one clause of two eager literals): the plan reports no prefilter."""
    seg, g, v = seg17
    for where in ("f <> %d" % v, "f IN (%d) OR f BETWEEN %d AND %d" % (v, v + 300, v + 600), "f IN (%d) OR g IN (70)" % v):
        q, plan, got = _run(_sql(v, where), [g], ON)
        assert plan["eq_prefilter"] == 0, (where, plan)
        assert_same(got, oracle.run_query(q, [seg]))


def test_stream_nt_gives_the_same_results(seg17):
    seg, g, v = seg17
    q, plan0, got0 = _run(_sql(v), [g], {"stream_nt": 0})
    _, plan1, got1 = _run(_sql(v), [g], {"stream_nt": 1})
    _, plan_auto, _ = _run(_sql(v), [g])
    assert (plan0["stream_nt"], plan1["stream_nt"], plan_auto["stream_nt"]) == (0, 1, 0)  # (auto: the table fits the caches)
    assert (plan0["eq_prefilter"], plan1["eq_prefilter"], plan_auto["eq_prefilter"]) == (0, 1, 0)  # (auto follows nt)
    exp = oracle.run_query(q, [seg])
    assert_same(got0, exp)
    assert_same(got1, exp)
    # a range (the hoisted loop without the prefilter) and a two-clause filter (the other hoisted loop)
    for where in ("f BETWEEN %d AND %d" % (v, v + 30), "f IN (%d) AND g IN (0, 10, 20, 30)" % v):
        q, _, a = _run(_sql(v, where), [g], {"stream_nt": 0})
        _, p, b = _run(_sql(v, where), [g], {"stream_nt": 1})
        assert p["stream_nt"] == 1
        exp = oracle.run_query(q, [seg])
        assert_same(a, exp)
        assert_same(b, exp)


def test_entries_scanned_in_filter_is_the_same_with_the_prefilter(seg17):
    seg, g, v = seg17
    where = "f IN (%d) AND g IN (0, 10, 20, 30)" % v
    q, plan1, got1 = _run(_sql(v, where), [g], ON, execution_stats=True)
    _, plan0, got0 = _run(_sql(v, where), [g], {"eq_prefilter": 0}, execution_stats=True)
    exp = oracle.run_query(q, [seg])
    assert_same(got1, exp)
    assert_same(got0, exp)
    assert plan1["eq_prefilter"] == 1 and plan0["eq_prefilter"] == 0, (plan1, plan0)
    assert got1.num_entries_scanned_in_filter == got0.num_entries_scanned_in_filter > 0
    assert got1.num_entries_scanned_post_filter == got0.num_entries_scanned_post_filter


# ------------------------------------------------------------------ reset

RESET_QUERIES = (
    # MIN + MAX + SUM group-by: zeroed sums next to MIN / MAX identities in one accumulator block
    "SELECT g, MIN(s), MAX(s), SUM(s) FROM t WHERE f BETWEEN 0 AND 3000 GROUP BY g LIMIT 100",
    # the equality query with a second clause: the scan counts the leap statistics (leap header beside the block)
    None,
)


def _double(res):
    """res scanned twice into one block: SUMs and numDocsScanned double, MIN / MAX stay."""
    out = {}
    for k, vals in res.groups.items():
        out[k] = [v if a.function in ("MIN", "MAX") else 2 * v for a, v in zip(res.aggregations, vals)]
    return out


@pytest.mark.parametrize("external", [False, True], ids=["own_block", "external_block"])
@pytest.mark.parametrize("which", [0, 1], ids=["min_max_sum", "equality_leap"])
@pytest.mark.parametrize("fused", [1, 0], ids=["one_launch", "memsets"])
def test_reset_semantics(seg17, which, external, fused):
    seg, g, v = seg17
    sql = RESET_QUERIES[which] or _sql(v, "f IN (%d) AND g IN (0, 10, 20, 30)" % v)
    q = parse_sql(sql)
    exp = oracle.run_query(q, [seg])
    assert exp.groups
    ex = GpuQueryExecutor(q, [g], tuning=dict(GRID, reset_fused=fused, **ON))
    keep = None
    try:
        if which == 1:
            assert int(L.lib().pa_query_leap_leaf(ex.handle)) >= 0  # leap mode
            assert ex.stats()["plan"]["eq_prefilter"] == 1
        if external:
            n = int(L.lib().pa_query_accumulator_bytes(ex.handle))
            keep = torch.full((n + 512,), 0x5A, dtype=torch.uint8, device="cuda")  # (a dirty block: reset must clean it)
            base = keep.data_ptr() + (-keep.data_ptr()) % 256
            L.check(L.lib().pa_query_set_accumulator_buffer(ex.handle, base, n), "set_accumulator_buffer")
        # reset, fetch: empty
        ex.reset()
        r = ex.fetch(execution_stats=False)
        assert r.num_docs_scanned == 0 and not r.groups
        # execute twice: the same as once
        ex.execute()
        ex.execute()
        assert_same(ex.fetch(execution_stats=False), exp)
        # reset, scan, scan: doubled sums, MIN / MAX unchanged
        ex.reset()
        ex.scan()
        ex.scan()
        r = ex.fetch(execution_stats=False)
        assert r.num_docs_scanned == 2 * exp.num_docs_scanned
        assert r.groups == _double(exp)
        # and a reset after that leaves nothing behind
        ex.execute()
        assert_same(ex.fetch(execution_stats=False), exp)
    finally:
        ex.close()
