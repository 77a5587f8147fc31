"""Exact PERCENTILE / PERCENTILEMV on the GPU (value histograms through the C-ABI).

The reference's 25 golden results; parity of the intermediate ValueHistograms with numpy multisets over synthetic
segments with different dictionaries (value remaps) under the default plan, global atomics and LDS bins; the GPU rank
select (pa_query_percentiles) against reduce.final_value; invariants against the oracle (which computes no percentile)
for filters numpy cannot evaluate: every histogram's total is COUNT(*) / COUNTMV, percentile 0 is MIN, percentile 100
is MAX, the group sets are equal, also under numGroupsLimit; the smallest shapes that can still go wrong; refusals.
Everything is exact: bins are integer counts and the results are dictionary values.
"""
import json
import math
import os

import numpy as np
import pytest

import oracle
from conftest import GOLDEN, rows_match
from pinot_amd import _lib as L
from pinot_amd import parse_sql
from pinot_amd.engine import GpuQueryExecutor, GpuSegment, UnsupportedQuery, ValueHistogram
from pinot_amd.reduce import final_result_table, final_value, merge_intermediate, server_trim
from pinot_amd.segment import create_segment

pytestmark = pytest.mark.gpu

PERCENTILES = (0, 50, 90, 99.9, 100)
SCHEMA = {"g": "INT", "i": "INT", "l": "LONG", "f": "FLOAT", "d": "DOUBLE", "s": "STRING", "tags": "INT", "r": "LONG"}


def synth(seed, n):
    """12 group keys g, INT / LONG / FLOAT / DOUBLE dictionary columns whose dictionaries differ with the seed, a STRING
    column, an MV INT column tags (1..4 values per doc), a raw LONG column r. Returns (segment, its column data)."""
    rng = np.random.default_rng(seed)
    data = {
        "g": (rng.integers(0, 12, size=n) * 5 + 3).astype(np.int32),
        "i": rng.integers(-40 - seed, 41 + 2 * seed, size=n).astype(np.int32),
        "l": (rng.integers(0, 90 + seed, size=n).astype(np.int64) - 30) * 5_000_000_000,
        "f": (rng.integers(0, 70 + seed, size=n) * 0.37 - 9).astype(np.float32),
        "d": rng.integers(0, 110 + seed, size=n) * 1.1 - 50.0,
        "s": np.array(["ab", "ac", "b", "cab", "abc" + str(seed)])[rng.integers(0, 5, size=n)],
        "tags": [(rng.integers(0, 30 + seed % 3, size=k) * 7 + 100).astype(np.int32) for k in rng.integers(1, 5, size=n)],
        "r": rng.integers(0, 1000, size=n).astype(np.int64),
    }
    return create_segment("pct%d" % seed, data, SCHEMA, no_dictionary_columns=("r",), multi_value_columns=("tags",)), data


@pytest.fixture(scope="module")
def table():
    """Two segments of 40,000 and 9,000 docs (different dictionaries), resident on the GPU; shared, never changed."""
    parts = [synth(3, 40000), synth(4, 9000)]
    gsegs = [GpuSegment(s) for s, _ in parts]
    yield [s for s, _ in parts], [d for _, d in parts], gsegs
    for g in gsegs:
        g.close()


def run(sql, gsegs, flags=0, percentiles=False):
    ex = GpuQueryExecutor(parse_sql(sql), gsegs, flags=flags)
    try:
        ex.execute()
        res = ex.fetch(execution_stats=False)
        sel = ex.percentiles() if percentiles else None
        plan = ex.stats()["plan"]["strategy"]
        return res, sel, plan, ex
    finally:
        ex.close()


def numpy_histograms(datas, column, mask_of, grouped):
    """The multiset of `column` over the docs mask_of(data) keeps: {g: ValueHistogram} or one ValueHistogram."""
    keys, vals = [], []
    for d in datas:
        m = mask_of(d)
        if column == "tags":
            rows = [t for t, keep in zip(d["tags"], m) if keep]
            vals.append(np.concatenate(rows).astype(np.float64) if rows else np.zeros(0))
            keys.append(np.repeat(d["g"][m], [len(t) for t in rows]))
        else:
            vals.append(d[column][m].astype(np.float64))
            keys.append(d["g"][m])
    keys, vals = np.concatenate(keys), np.concatenate(vals)
    if not grouped:
        return ValueHistogram.from_values(vals)
    return {int(k): ValueHistogram.from_values(vals[keys == k]) for k in np.unique(keys)}


COLUMNS = ("i", "l", "f", "d", "tags")
SELECT = ", ".join("PERCENTILE%s(%s, 50)" % ("MV" if c == "tags" else "", c) for c in COLUMNS)
FILTERS = {"": lambda d: np.ones(len(d["i"]), dtype=bool), " WHERE i > 0": lambda d: d["i"] > 0,
           " WHERE i > 100000": lambda d: d["i"] > 100000}


@pytest.fixture(scope="module")
def numpy_reference(table):
    _, datas, _ = table
    return {(w, c, grouped): numpy_histograms(datas, c, FILTERS[w], grouped)
            for w in FILTERS for c in COLUMNS for grouped in (False, True)}


# ------------------------------------------------------------------ the reference's golden results
def test_golden_percentile_cases_gpu(golden_segment):
    with open(os.path.join(GOLDEN, "sv_percentile_queries.json")) as f:
        spec = json.load(f)
    g = GpuSegment(golden_segment)
    failures = []
    try:
        for case in spec["cases"]:
            q = parse_sql(case["sql"])
            ex = GpuQueryExecutor(q, [g, g])  # one server = 2 copies of the segment
            ex.execute()
            server = ex.fetch(execution_stats=True)
            ex.close()
            broker = merge_intermediate([server_trim(server, q)] * 2)
            got = final_result_table(broker, q)
            if not rows_match(got, case["rows"], case["delta"]):
                failures.append((case["source"], got[:3], case["rows"][:3]))
            stats = [broker.num_docs_scanned, broker.num_entries_scanned_in_filter,
                     broker.num_entries_scanned_post_filter, broker.num_total_docs]
            if stats != case["stats"]:
                failures.append((case["source"], "stats", stats, case["stats"]))
    finally:
        g.close()
    assert len(spec["cases"]) == 25 and not failures, failures


# ------------------------------------------------------------------ synthetic parity with numpy multisets
@pytest.mark.parametrize("flags, strategy", [(0, None), (L.PA_QF_FORCE_GLOBAL, "global"), (L.PA_QF_FORCE_LDS, "lds")])
@pytest.mark.parametrize("where", list(FILTERS))
def test_histograms_equal_numpy_multisets(table, numpy_reference, flags, strategy, where):
    _, _, gsegs = table
    res, _, plan, _ = run("SELECT %s FROM t%s" % (SELECT, where), gsegs, flags)
    assert strategy is None or plan == strategy
    for c, h in zip(COLUMNS, res.row):
        assert h == numpy_reference[(where, c, False)], (c, h)
    res, _, plan, _ = run("SELECT g, %s FROM t%s GROUP BY g LIMIT 100" % (SELECT, where), gsegs, flags)
    assert strategy is None or plan == strategy
    exp = numpy_reference[(where, "i", True)]
    assert set(res.groups) == {(k,) for k in exp}
    for (k,), hs in res.groups.items():
        for c, h in zip(COLUMNS, hs):
            assert h == numpy_reference[(where, c, True)][k], (k, c, h)


@pytest.mark.parametrize("column", ["d", "tags"])
@pytest.mark.parametrize("where", list(FILTERS))
def test_gpu_rank_select_agrees_with_final_value(table, numpy_reference, column, where):
    _, _, gsegs = table
    fn = "PERCENTILEMV" if column == "tags" else "PERCENTILE"
    select = ", ".join("%s(%s, %s)" % (fn, column, p) for p in PERCENTILES)
    for group_by in ("", " GROUP BY g LIMIT 100"):
        res, (keys, sel), _, ex = run("SELECT %s FROM t%s%s" % (select, where, group_by), gsegs, percentiles=True)
        assert len(ex.pa_aggs) == 1  # five percentiles of one column: one histogram accumulator
        rows = list(res.groups.values()) if group_by else [res.row]
        assert len(keys) == len(rows) and set(sel) == set(range(len(PERCENTILES)))
        for ai, agg in enumerate(ex.query.aggregations):
            exp = [final_value(agg, row[ai]) for row in rows]
            assert sel[ai].tolist() == exp, (agg, sel[ai], exp)
        if not group_by:  # (and final_value itself against the sorted multiset)
            h = numpy_reference[(where, column, False)]
            allv = np.repeat(h.values, h.counts)
            for ai, p in enumerate(PERCENTILES):
                exp = -math.inf if not len(allv) else allv[len(allv) - 1 if p == 100 else int(float(len(allv)) * p / 100)]
                assert sel[ai][0] == exp


# ------------------------------------------------------------------ invariants against the unchanged oracle
ORACLE_FILTERS = ["i IN (1, 5, 9, -3, 22)", "i > 10 OR l < 0", "REGEXP_LIKE(s, '^a.*')", "tags = 121",
                  "tags IN (107, 128) AND i <> 4"]


@pytest.mark.parametrize("option", ["", " OPTION(numGroupsLimit=5)"])
@pytest.mark.parametrize("flt", ORACLE_FILTERS)
def test_invariants_against_oracle(table, flt, option):
    segs, _, gsegs = table
    tail = " FROM t WHERE %s GROUP BY g LIMIT 100%s" % (flt, option)
    res, _, _, _ = run("SELECT g, PERCENTILE(d, 0), PERCENTILE(d, 100), PERCENTILEMV(tags, 0), PERCENTILEMV(tags, 100)"
                       + tail, gsegs)
    q = parse_sql("SELECT g, COUNT(*), MIN(d), MAX(d), COUNTMV(tags), MINMV(tags), MAXMV(tags)" + tail)
    exp = oracle.run_query(q, segs)
    assert exp.groups and set(res.groups) == set(exp.groups)
    assert res.num_docs_scanned == exp.num_docs_scanned
    assert res.num_groups_limit_reached == exp.num_groups_limit_reached == bool(option)
    aggs = parse_sql("SELECT PERCENTILE(d, 0), PERCENTILE(d, 100), PERCENTILEMV(tags, 0), PERCENTILEMV(tags, 100) FROM t"
                     ).aggregations
    for k, (count, dmin, dmax, countmv, tmin, tmax) in exp.groups.items():
        d0, d100, t0, t100 = res.groups[k]
        assert d0 == d100 and t0 == t100  # (one accumulator per column)
        assert d0.total == count and t0.total == countmv, (k, d0.total, count, t0.total, countmv)
        assert [final_value(a, h) for a, h in zip(aggs, (d0, d100, t0, t100))] == [dmin, dmax, tmin, tmax]


# ------------------------------------------------------------------ the smallest shapes that can still go wrong
def _one_segment(n, columns, schema, **kw):
    seg = create_segment("shape", columns, schema, **kw)
    return seg, GpuSegment(seg)


@pytest.mark.parametrize("flags", [0, L.PA_QF_FORCE_GLOBAL, L.PA_QF_FORCE_LDS])
def test_cardinality_one_and_three(flags):
    n = 5000
    rng = np.random.default_rng(11)
    three = np.array([7, 8, 9], dtype=np.int32)[rng.integers(0, 3, size=n)]
    seg, g = _one_segment(n, {"one": np.full(n, 42, dtype=np.int32), "three": three}, {"one": "INT", "three": "INT"})
    try:
        res, (_, sel), _, ex = run("SELECT PERCENTILE(one, 50), PERCENTILE(three, 50) FROM t", [g], flags,
                                   percentiles=True)
        h1, h3 = res.row
        assert h1 == ValueHistogram([42.0], [n])  # every doc adds to one bin
        assert h3 == ValueHistogram.from_values(three)  # stride 4: the padding bin stays 0
        assert sel[0][0] == 42.0 and sel[1][0] == final_value(ex.query.aggregations[1], h3)
        # the pairs as the library returns them: a non-zero padding bin would come back as value id 3
        ex2 = GpuQueryExecutor(parse_sql("SELECT PERCENTILE(three, 50) FROM t"), [g], flags=flags)
        try:
            ex2.execute()
            ends, ids, counts = np.zeros(1, np.int64), np.full(8, -1, np.int32), np.zeros(8, np.int64)
            lib = L.lib()
            assert lib.pa_query_fetch_histogram(ex2.handle, None, 0, 1, 0, ends.ctypes.data, None, None) == 3
            assert lib.pa_query_fetch_histogram(ex2.handle, None, 0, 1, 8, ends.ctypes.data, ids.ctypes.data,
                                                counts.ctypes.data) == 3
            assert ends.tolist() == [3] and ids.tolist() == [0, 1, 2, -1, -1, -1, -1, -1]
            assert counts[:3].tolist() == np.bincount(three - 7, minlength=3).tolist()
            # a capacity below the pair count: only that many pairs are written, the count is still returned
            ids[:] = -1
            assert lib.pa_query_fetch_histogram(ex2.handle, None, 0, 1, 2, ends.ctypes.data, ids.ctypes.data,
                                                counts.ctypes.data) == 3
            assert ids.tolist() == [0, 1, -1, -1, -1, -1, -1, -1]
        finally:
            ex2.close()
    finally:
        g.close()


def test_cardinality_50000_ungrouped():
    """~50,000 distinct values over 60,000 docs: the bins cannot fit LDS, a row spans ~200 passes of the count, compaction
    and select kernels."""
    n = 60000
    rng = np.random.default_rng(12)
    ids = rng.permutation(np.concatenate([np.arange(50000), rng.integers(0, 50000, size=n - 50000)]))
    wide = ids.astype(np.int64) * 3 - 70000  # every one of 50,000 values at least once
    seg, g = _one_segment(n, {"wide": wide}, {"wide": "LONG"})
    try:
        select = ", ".join("PERCENTILE(wide, %s)" % p for p in PERCENTILES)
        res, (_, sel), plan, ex = run("SELECT %s FROM t" % select, [g], percentiles=True)
        assert plan == "global" and len(ex.pa_aggs) == 1
        exp = ValueHistogram.from_values(wide)
        assert len(exp.values) == 50000 and res.row[0] == exp
        srt = np.sort(wide.astype(np.float64))
        for ai, p in enumerate(PERCENTILES):
            assert sel[ai][0] == srt[n - 1 if p == 100 else int(float(n) * p / 100)]
    finally:
        g.close()


@pytest.mark.parametrize("flags", [0, L.PA_QF_FORCE_GLOBAL])
def test_grouped_12_by_600_with_zero_doc_segment(flags):
    n = 30000
    rng = np.random.default_rng(13)
    k = (rng.integers(0, 12, size=n) + 1).astype(np.int32)
    v = rng.integers(0, 600, size=n).astype(np.int32) * 2
    schema = {"k": "INT", "v": "INT"}
    seg, g = _one_segment(n, {"k": k, "v": v}, schema)
    empty = GpuSegment(create_segment("empty", {"k": np.zeros(0, np.int32), "v": np.zeros(0, np.int32)}, schema))
    try:
        res, (keys, sel), _, ex = run("SELECT k, PERCENTILE(v, 50), PERCENTILE(v, 90), PERCENTILE(v, 100) FROM t "
                                      "GROUP BY k LIMIT 100", [g, empty], flags, percentiles=True)
        assert len(ex.pa_aggs) == 1  # three percentiles of one column: one histogram aggregation in the spec
        assert res.num_total_docs == n and set(res.groups) == {(int(x),) for x in np.unique(k)}
        for gi, (key,) in enumerate(res.groups):
            exp = ValueHistogram.from_values(v[k == key])
            assert res.groups[(key,)][0] == exp
            for ai, agg in enumerate(ex.query.aggregations):
                assert sel[ai][gi] == final_value(agg, exp)
    finally:
        g.close()
        empty.close()


def test_filter_matching_nothing(table):
    _, _, gsegs = table
    res, (keys, sel), _, _ = run("SELECT g, PERCENTILE(d, 50) FROM t WHERE i > 100000 GROUP BY g LIMIT 10", gsegs,
                                 percentiles=True)
    assert res.groups == {} and len(keys) == 0 and len(sel[0]) == 0
    res, (keys, sel), _, ex = run("SELECT PERCENTILE(d, 50), PERCENTILEMV(tags, 99.9) FROM t WHERE i > 100000", gsegs,
                                  percentiles=True)
    assert [h.total for h in res.row] == [0, 0]
    assert [final_value(a, h) for a, h in zip(ex.query.aggregations, res.row)] == [-math.inf, -math.inf]
    assert sel[0].tolist() == [-math.inf] and sel[1].tolist() == [-math.inf]


# ------------------------------------------------------------------ refusals
def test_refusals(table):
    _, _, gsegs = table
    with pytest.raises(UnsupportedQuery, match="raw"):
        GpuQueryExecutor(parse_sql("SELECT PERCENTILE(r, 50) FROM t"), gsegs)
    with pytest.raises(UnsupportedQuery):
        GpuQueryExecutor(parse_sql("SELECT PERCENTILE(s, 50) FROM t"), gsegs)
    with pytest.raises(L.PinotAmdError, match="hashed key space"):  # GROUP BY a raw column: hashed keys
        GpuQueryExecutor(parse_sql("SELECT r, PERCENTILE(d, 50) FROM t GROUP BY r LIMIT 10"), gsegs)
    # the device is still usable
    res, _, _, _ = run("SELECT PERCENTILE(d, 50) FROM t", gsegs)
    assert res.row[0].total == 49000


def test_percentile_arguments_checked_by_the_library(table):
    _, _, gsegs = table
    ex = GpuQueryExecutor(parse_sql("SELECT PERCENTILE(d, 50), COUNT(*) FROM t"), gsegs)
    try:
        ex.execute()
        lib = L.lib()
        out = np.zeros(2, dtype=np.int32)
        for bad in (-0.5, 100.5, float("nan")):
            ps = np.array([50.0, bad])
            assert lib.pa_query_percentiles(ex.handle, None, 0, 1, 2, ps.ctypes.data, out.ctypes.data) == -1  # PA_EINVAL
        ps = np.array([50.0])
        assert lib.pa_query_percentiles(ex.handle, None, 1, 1, 1, ps.ctypes.data, out.ctypes.data) == -1  # COUNT(*)
        assert lib.pa_query_percentiles(ex.handle, None, 0, 7, 1, ps.ctypes.data, out.ctypes.data) == -1  # 1 group
        assert lib.pa_query_percentiles(ex.handle, None, 0, 1, 1, ps.ctypes.data, out.ctypes.data) == 0
    finally:
        ex.close()
