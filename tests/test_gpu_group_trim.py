"""Group trim on the GPU (pa_query_fetch_trimmed, pa_trim.hip) through the engine: fetch(server_trim=True) is exactly
reduce.server_trim(fetch(), query) — keys, intermediate values, statistics, numGroupsLimitReached — and, where the
oracle runs the query, server_trim of the oracle's block.

Metrics are INT values (negative ones included) and DOUBLE multiples of 1/8, so every sum is exact in double whatever
the order of the additions: the comparisons below are all exact.
"""
import numpy as np
import pytest

import oracle
from conftest import golden_rows, rows_match
from pinot_amd import _lib as L
from pinot_amd import parse_sql
from pinot_amd import trim as TR
from pinot_amd.engine import GpuQueryExecutor, GpuSegment
from pinot_amd.reduce import final_result_table, merge_intermediate, server_trim
from pinot_amd.segment import create_segment
from synth import make_segment
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu


def trim_segment(seed, n, c1, c2, leave_out=None, mv=False):
    """g1 INT (c1 values) and g2 STRING (c2 values) dimensions, mi INT and md DOUBLE (eighths) metrics, v for the
    sketches, optionally the MV column tags. leave_out = (i, k): the segment never draws the pool values whose index is
    i modulo k, so segments get dictionaries of their own (table-wide remaps) whose union is still the whole pool."""
    rng = np.random.default_rng(seed)
    p1 = np.arange(c1, dtype=np.int32) * 3 - 40
    p2 = np.array(["s%04d%s" % (i, "y" * (i % 3)) for i in range(c2)])
    i1, i2 = np.arange(c1), np.arange(c2)
    if leave_out is not None:
        i1, i2 = i1[i1 % leave_out[1] != leave_out[0]], i2[i2 % leave_out[1] != leave_out[0]]
    data = {"g1": p1[rng.choice(i1, size=n)], "g2": p2[rng.choice(i2, size=n)],
            "mi": rng.integers(-500, 500, size=n).astype(np.int32),
            "md": rng.integers(-4000, 4000, size=n).astype(np.float64) / 8.0,
            "v": rng.integers(0, 200, size=n).astype(np.int32)}
    schema = {"g1": "INT", "g2": "STRING", "mi": "INT", "md": "DOUBLE", "v": "INT"}
    mvc = ()
    if mv:
        data["tags"] = [(rng.integers(0, 60, size=k) * 7 + 100).astype(np.int32) for k in rng.integers(1, 4, size=n)]
        schema["tags"] = "INT"
        mvc = ("tags",)
    return create_segment("trim%d" % seed, data, schema, multi_value_columns=mvc)


def same_block(got, want):
    assert set(got.groups) == set(want.groups), sorted(set(got.groups) ^ set(want.groups))[:5]
    assert got.groups == want.groups and list(got.groups) == list(want.groups)  # (values, and the key order too)
    assert got.row == want.row
    assert (got.num_docs_scanned, got.num_total_docs, got.num_entries_scanned_in_filter,
            got.num_entries_scanned_post_filter, got.num_groups_limit_reached) == (
        want.num_docs_scanned, want.num_total_docs, want.num_entries_scanned_in_filter,
        want.num_entries_scanned_post_filter, want.num_groups_limit_reached)


def check(sql, segs, gsegs, flags=0, device=True, ora=None, use_oracle=True, strategy=None):
    """The defining property for one query; returns (trimmed block, last_trim). ora: the oracle's block of a query with
    the same aggregations, filter and GROUP BY (the ORDER BY and LIMIT do not change it), computed once by the caller."""
    q = parse_sql(sql)
    ex = GpuQueryExecutor(q, gsegs, flags=flags)
    try:
        if strategy is not None:
            assert ex.stats()["plan"]["strategy"] == strategy
        ex.execute()
        want = server_trim(ex.fetch(), q)
        got = ex.fetch(server_trim=True)
        lt = dict(ex.last_trim)
    finally:
        ex.close()
    same_block(got, want)
    assert lt["device"] is device, (sql, lt)
    assert lt["kept"] == len(got.groups) == min(lt["groups"], TR.trim_size(q)), (sql, lt)
    if use_oracle:
        exp = server_trim(ora if ora is not None else oracle.run_query(q, segs), q)
        assert_same(got, exp)
        assert len(got.groups) == len(exp.groups)
    return got, lt


# ------------------------------------------------------------------ the reference's golden cases
def test_golden_order_by_cases(golden_spec, golden_segment):
    """Every GROUP BY ... ORDER BY case of the golden file with the trim on the server's GPU: the broker rows are the
    reference's. Shapes the device refuses (ORDER BY DISTINCTCOUNT / HLL / DISTINCTSUM / DISTINCTAVG) take the host trim."""
    g = GpuSegment(golden_segment)
    failures, ran, on_device = [], 0, 0
    try:
        for case in golden_spec["cases"]:
            q = parse_sql(case["sql"])
            if not (q.group_by and q.order_by):
                continue
            ran += 1
            ex = GpuQueryExecutor(q, [g, g])  # one server = 2 copies of the segment
            try:
                ex.execute()
                server = ex.fetch(server_trim=True)
                lt = dict(ex.last_trim)
                same_block(server, server_trim(ex.fetch(), q))
                try:
                    TR.lower_order_by(q, ex.agg_map, ex.hashed)
                    refused = False
                except TR.HostTrim:
                    refused = True
            finally:
                ex.close()
            assert lt["device"] is (not refused), (case["source"], lt)
            on_device += lt["device"]
            got = final_result_table(merge_intermediate([server] * 2), q)
            if case["rows"] is not None and not rows_match(golden_rows(got, case), case["rows"], case["delta"]):
                failures.append((case["source"], got[:3], case["rows"][:3]))
    finally:
        g.close()
    assert ran >= 39 and on_device >= 25, (ran, on_device)
    assert not failures, failures


# ------------------------------------------------------------------ small key space: 37 x 61
AGGS = "COUNT(*), SUM({m}), MIN({m}), MAX({m}), AVG({m}), MINMAXRANGE({m})"


@pytest.fixture(scope="module")
def small():
    """37 x 61 = 2257 keys (two 2048-key compaction blocks, the second ragged), ~20k docs in 3 ragged segments with
    dictionaries of their own; the oracle's block per metric, computed once."""
    segs = [trim_segment(500 + i, n, 37, 61, leave_out=(i, 7)) for i, n in enumerate((9973, 7001, 3037))]
    gsegs = [GpuSegment(s) for s in segs]
    ora = {m: oracle.run_query(parse_sql("SELECT g1, g2, %s FROM t GROUP BY g1, g2 LIMIT 100000" % AGGS.format(m=m)),
                               segs) for m in ("mi", "md")}
    assert len(ora["mi"].groups) > 2100
    yield segs, gsegs, ora
    for g in gsegs:
        g.close()


# (limit, minServerGroupTrimSize, trim = max(5 limit, minServerGroupTrimSize)): trims of 5, 64 and 2049, and what the
# limits 13 and 410 give on their own
@pytest.mark.parametrize("limit,min_trim,trim", [(1, 1, 5), (12, 64, 64), (13, 1, 65), (409, 2049, 2049),
                                                 (410, 2049, 2050), (410, 1, 2050)])
def test_small_key_space_trims(small, limit, min_trim, trim):
    segs, gsegs, ora = small
    sql = ("SELECT g1, g2, %s FROM t GROUP BY g1, g2 ORDER BY SUM(mi) DESC LIMIT %d OPTION(minServerGroupTrimSize=%d)"
           % (AGGS.format(m="mi"), limit, min_trim))
    got, lt = check(sql, segs, gsegs, ora=ora["mi"])
    assert len(got.groups) == trim and lt["groups"] == len(ora["mi"].groups)


@pytest.mark.parametrize("under", [0, 1])
def test_trim_of_all_groups_and_all_but_one(small, under):
    segs, gsegs, ora = small
    n = len(ora["mi"].groups)
    sql = ("SELECT g1, g2, %s FROM t GROUP BY g1, g2 ORDER BY AVG(mi), g2 DESC LIMIT 1 "
           "OPTION(minServerGroupTrimSize=%d)" % (AGGS.format(m="mi"), n - under))
    got, lt = check(sql, segs, gsegs, ora=ora["mi"])
    assert len(got.groups) == n - under and lt == {"device": True, "groups": n, "kept": n - under}


def test_fewer_groups_than_the_trim_is_the_plain_fetch(small):
    segs, gsegs, _ = small
    sql = ("SELECT g1, g2, %s FROM t WHERE g1 < -30 GROUP BY g1, g2 ORDER BY COUNT(*) DESC LIMIT 10"
           % AGGS.format(m="mi"))
    got, lt = check(sql, segs, gsegs)
    assert 100 < lt["groups"] == lt["kept"] < 5000
    q = parse_sql(sql)
    ex = GpuQueryExecutor(q, gsegs)
    try:
        ex.execute()
        same_block(got, ex.fetch())
    finally:
        ex.close()


TERM_KINDS = ["g1", "g2", "COUNT(*)", "SUM({m})", "MIN({m})", "MAX({m})", "AVG({m})", "MINMAXRANGE({m})"]


@pytest.mark.parametrize("desc", ["", " DESC"], ids=["asc", "desc"])
@pytest.mark.parametrize("metric", ["mi", "md"])
def test_every_term_kind(small, metric, desc):
    segs, gsegs, ora = small
    for term in TERM_KINDS:
        sql = ("SELECT g1, g2, %s FROM t GROUP BY g1, g2 ORDER BY %s%s LIMIT 8 OPTION(minServerGroupTrimSize=1)"
               % (AGGS.format(m=metric), term.format(m=metric), desc))
        got, _ = check(sql, segs, gsegs, ora=ora[metric])
        assert len(got.groups) == 40


@pytest.mark.parametrize("metric", ["mi", "md"])
def test_three_term_order(small, metric):
    segs, gsegs, ora = small
    sql = ("SELECT g1, g2, %s FROM t GROUP BY g1, g2 ORDER BY g2 DESC, SUM(%s), AVG(%s) DESC LIMIT 21 "
           "OPTION(minServerGroupTrimSize=1)" % (AGGS.format(m=metric), metric, metric))
    got, _ = check(sql, segs, gsegs, ora=ora[metric])
    assert len(got.groups) == 105


def test_no_order_by(small):
    segs, gsegs, ora = small
    got, _ = check("SELECT g1, g2, %s FROM t GROUP BY g1, g2 LIMIT 7" % AGGS.format(m="mi"), segs, gsegs, ora=ora["mi"])
    assert set(got.groups) == set(sorted(ora["mi"].groups)[:7])


def test_selected_sketches_are_gathered_for_the_kept_groups(small):
    segs, gsegs, _ = small
    got, _ = check("SELECT g1, g2, SUM(mi), DISTINCTCOUNTHLL(v), DISTINCTCOUNT(v) FROM t GROUP BY g1, g2 "
                   "ORDER BY SUM(mi) DESC LIMIT 13 OPTION(minServerGroupTrimSize=1)", segs, gsegs)
    assert len(got.groups) == 65
    assert all(len(vals[2]) > 0 for vals in got.groups.values())  # (the value sets came with their groups)


@pytest.mark.parametrize("sql", [
    "SELECT g1, COUNT(*), DISTINCTCOUNT(v) FROM t GROUP BY g1 ORDER BY DISTINCTCOUNT(v) DESC, g1 LIMIT 2 "
    "OPTION(minServerGroupTrimSize=1)",
    "SELECT g1, COUNT(*), PERCENTILE50(mi) FROM t GROUP BY g1 ORDER BY COUNT(*) LIMIT 2 OPTION(minServerGroupTrimSize=1)",
    "SELECT g1, COUNT(*), SUM(mi) FILTER (WHERE v < 50) FROM t GROUP BY g1 ORDER BY COUNT(*) LIMIT 2 "
    "OPTION(minServerGroupTrimSize=1)",
    "SELECT g1, COUNT(*) FROM t GROUP BY g1, g2, v ORDER BY g1, g2, v, COUNT(*), g1 DESC LIMIT 2 "
    "OPTION(minServerGroupTrimSize=1)",
], ids=["order_by_distinctcount", "value_histogram", "aggregation_filter", "five_terms"])
def test_refused_shapes_take_the_host_trim(small, sql):
    segs, gsegs, _ = small
    got, lt = check(sql, segs, gsegs, device=False, use_oracle=False)
    assert len(got.groups) == 10 < lt["groups"]


def test_library_refuses_what_the_header_says(small):
    """pa_query_fetch_trimmed itself answers PA_EUNSUPPORTED for a term over a sketch and for too many terms, and
    PA_EINVAL for an index outside the query."""
    segs, gsegs, _ = small
    q = parse_sql("SELECT g1, COUNT(*), SUM(mi), DISTINCTCOUNTHLL(v) FROM t GROUP BY g1 LIMIT 10")
    ex = GpuQueryExecutor(q, gsegs)
    try:
        ex.execute()
        hll = ex.agg_map[2]
        for terms, code in (([(L.PA_TRIM_AGG, hll, 0, 0)], L.PA_EUNSUPPORTED),
                            ([(L.PA_TRIM_AGG, 99, 0, 0)], L.PA_EINVAL),
                            ([(L.PA_TRIM_KEY_COLUMN, 1, 0, 0)], L.PA_EINVAL),
                            ([(L.PA_TRIM_AVG, ex.agg_map[0], 0, 0)], L.PA_EINVAL)):
            with pytest.raises(L.PinotAmdError) as e:
                ex.fetch_arrays(trim_spec=TR.build_spec(terms, 3))
            assert e.value.code == code, terms
        spec = TR.build_spec([], 3)
        spec.num_terms = 5
        with pytest.raises(L.PinotAmdError) as e:
            ex.fetch_arrays(trim_spec=spec)
        assert e.value.code == L.PA_EUNSUPPORTED
    finally:
        ex.close()


@pytest.mark.parametrize("flags", [0, L.PA_QF_FORCE_GLOBAL], ids=["default_plan", "force_global"])
def test_accumulation_paths(small, flags):
    segs, gsegs, ora = small
    sql = ("SELECT g1, g2, %s FROM t GROUP BY g1, g2 ORDER BY MINMAXRANGE(md) DESC, SUM(md) LIMIT 30 "
           "OPTION(minServerGroupTrimSize=1)" % AGGS.format(m="md"))
    got, _ = check(sql, segs, gsegs, flags=flags, ora=ora["md"])
    assert len(got.groups) == 150


def test_mv_group_by():
    segs = [trim_segment(520 + i, n, 9, 5, mv=True) for i, n in enumerate((6007, 2003))]
    gsegs = [GpuSegment(s) for s in segs]
    try:
        for order in ("COUNT(*) DESC", "SUM(mi)", "tags DESC"):
            got, lt = check("SELECT tags, COUNT(*), SUM(mi), MAX(md) FROM t GROUP BY tags ORDER BY %s LIMIT 3 "
                            "OPTION(minServerGroupTrimSize=1)" % order, segs, gsegs)
            assert len(got.groups) == 15 and lt["groups"] == 60
    finally:
        for g in gsegs:
            g.close()


# ------------------------------------------------------------------ large key space: 300 x 300
@pytest.fixture(scope="module")
def large():
    """300 x 300 = 90,000 keys (above the engine's 2^16 switch), 200k docs: most groups hold 1..3 docs."""
    segs = [trim_segment(540, 200_000, 300, 300)]
    gsegs = [GpuSegment(s) for s in segs]
    ora = oracle.run_query(parse_sql("SELECT g1, g2, COUNT(*), SUM(mi) FROM t GROUP BY g1, g2 LIMIT 1000000 "
                                     "OPTION(numGroupsLimit=2000000)"), segs)
    yield segs, gsegs, ora
    for g in gsegs:
        g.close()


@pytest.mark.parametrize("desc", [" DESC", ""], ids=["desc", "asc"])
def test_large_key_space_cut_inside_a_tie_class(large, desc):
    segs, gsegs, ora = large
    sql = ("SELECT g1, g2, COUNT(*), SUM(mi) FROM t GROUP BY g1, g2 ORDER BY COUNT(*)%s LIMIT 10 "
           "OPTION(numGroupsLimit=2000000)" % desc)
    got, lt = check(sql, segs, gsegs, ora=ora)
    assert lt["groups"] == len(ora.groups) > 70_000 and len(got.groups) == 5000
    counts = sorted(vals[0] for vals in got.groups.values())
    cut = counts[0] if desc else counts[-1]
    assert sum(1 for vals in ora.groups.values() if vals[0] == cut) > sum(1 for c in counts if c == cut) > 0


def test_partitioned_plan():
    """The accumulators of the partitioned aggregation (records partitioned by key range, aggregated per partition in
    LDS) under the trim, at the small size test_gpu_parity.test_partitioned_aggregation takes that plan."""
    cols = {"k1": ("INT", 700), "k2": ("LONG", 900), "m": ("INT", 5000)}
    segs = [make_segment(70 + i, n, cols) for i, n in enumerate((120011, 40009))]
    gsegs = [GpuSegment(s) for s in segs]
    try:
        got, lt = check("SELECT k1, k2, COUNT(*), SUM(m), MIN(m), MAX(m), AVG(m) FROM t GROUP BY k1, k2 "
                        "ORDER BY SUM(m) DESC, k1 LIMIT 20 OPTION(numGroupsLimit=2000000,minServerGroupTrimSize=100)",
                        segs, gsegs, strategy="partitioned")
        assert len(got.groups) == 100 and lt["groups"] > 50000
    finally:
        for g in gsegs:
            g.close()
