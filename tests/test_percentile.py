"""Exact PERCENTILE / PERCENTILEMV, host side: the accepted spellings, the ValueHistogram intermediate result (merge +
rank rule against a sorted array), the reference's 25 golden results at the reduce level, and the C-ABI's declarations.
"""
import json
import math
import os
import re

import numpy as np
import pytest

from pinot_amd import _lib as L
from pinot_amd import query as Q
from pinot_amd.engine import IntermediateResult, ValueHistogram
from pinot_amd.query import Aggregation, parse_sql
from pinot_amd.reduce import final_result_table, final_value, merge_intermediate, merge_value, server_trim

from conftest import GOLDEN, ROOT, rows_match

PERCENTILES = (0, 50, 99.9, 100)


def reference_percentile(values, p):
    """PercentileAggregationFunction.extractFinalResult over every value: sort, then the element at the rank."""
    v = np.sort(np.asarray(values, dtype=np.float64))
    if len(v) == 0:
        return -math.inf
    return float(v[len(v) - 1 if p == 100 else int(float(len(v)) * p / 100)])


# ------------------------------------------------------------------ spellings
@pytest.mark.parametrize("sql, function, percentile, version, name", [
    ("PERCENTILE50(column1)", "PERCENTILE", 50.0, 0, "percentile50(column1)"),
    ("percentile99(column1)", "PERCENTILE", 99.0, 0, "percentile99(column1)"),
    ("PERCENTILE100(column1)", "PERCENTILE", 100.0, 0, "percentile100(column1)"),
    ("PERCENTILE50MV(c)", "PERCENTILEMV", 50.0, 0, "percentile50mv(c)"),
    ("PERCENTILE(column1, 50)", "PERCENTILE", 50.0, 1, "percentile(column1, 50.0)"),
    ("PERCENTILE(column1, '50')", "PERCENTILE", 50.0, 1, "percentile(column1, 50.0)"),
    ("PERCENTILE(column1, 99.9)", "PERCENTILE", 99.9, 1, "percentile(column1, 99.9)"),
    ("PERCENTILE(column1, 0)", "PERCENTILE", 0.0, 1, "percentile(column1, 0.0)"),
    ("PERCENTILEMV(c, 50)", "PERCENTILEMV", 50.0, 1, "percentilemv(c, 50.0)"),
    ("PercentileMV(c, '99.9')", "PERCENTILEMV", 99.9, 1, "percentilemv(c, 99.9)"),
])
def test_spellings(sql, function, percentile, version, name):
    q = parse_sql("SELECT %s FROM testTable" % sql)
    column = "c" if function.endswith("MV") else "column1"
    assert q.aggregations == [Aggregation(function, column, percentile=percentile, version=version)]
    assert q.aggregations[0].result_name == name


@pytest.mark.parametrize("sql", ["PERCENTILE(c, 101)", "PERCENTILE(c, -1)", "PERCENTILEEST50(c)",
                                 "PERCENTILETDIGEST(c, 50)", "PERCENTILE101(c)", "PERCENTILEMV(c, 100.5)",
                                 "PERCENTILEKLL(c, 50)", "PERCENTILERAWEST50(c)", "PERCENTILE(c)", "PERCENTILE50(c, 3)"])
def test_rejected(sql):
    with pytest.raises(ValueError):
        parse_sql("SELECT %s FROM testTable" % sql)


@pytest.mark.parametrize("sql", ["PERCENTILEEST50(c)", "PERCENTILETDIGEST(c, 50)", "PERCENTILEKLL(c, 50)"])
def test_other_percentile_families_stay_unsupported(sql):
    with pytest.raises(ValueError, match="unsupported aggregation"):
        parse_sql("SELECT %s FROM testTable" % sql)


def test_order_by_matches_select_list():
    q = parse_sql("SELECT column11, percentile90(column6) FROM testTable GROUP BY column11 "
                  "ORDER BY PERCENTILE90(column6), column11 LIMIT 3")
    assert len(q.aggregations) == 1 and q.order_by[0].expr == q.aggregations[0]
    q = parse_sql("SELECT PERCENTILE(c, 50) AS v1 FROM t GROUP BY d ORDER BY v1 DESC LIMIT 1")
    assert q.order_by[0].expr == q.aggregations[0] and not q.order_by[0].asc
    # another percentile of the same column is another aggregation
    q = parse_sql("SELECT PERCENTILE50(c) FROM t GROUP BY d ORDER BY PERCENTILE90(c)")
    assert len(q.aggregations) == 2 and q.num_select_aggs == 1


def test_java_double_string():
    assert [Q.java_double_string(x) for x in (0, 50, 99.9, 100, 0.001, 0.0005, 12.5)] == \
        ["0.0", "50.0", "99.9", "100.0", "0.001", "5.0E-4", "12.5"]


# ------------------------------------------------------------------ ValueHistogram: merge + rank rule
@pytest.mark.parametrize("seed, n, card", [(1, 1, 1), (2, 7, 3), (3, 1000, 17), (4, 5000, 4000), (5, 999, 1)])
def test_value_histogram_against_sorted_array(seed, n, card):
    rng = np.random.default_rng(seed)
    pool = rng.normal(size=card) * 1e6
    a, b = pool[rng.integers(0, card, n)], pool[rng.integers(0, card, n // 2 + 1)]
    ha, hb = ValueHistogram.from_values(a), ValueHistogram.from_values(b)
    assert ha.total == len(a) and np.all(np.diff(ha.values) > 0) and np.all(ha.counts > 0)
    ab, ba = merge_value("PERCENTILE", ha, hb), merge_value("PERCENTILEMV", hb, ha)
    assert ab == ba == ValueHistogram.from_values(np.concatenate([a, b]))
    for p in PERCENTILES:
        for fn in ("PERCENTILE", "PERCENTILEMV"):
            agg = Aggregation(fn, "c", percentile=float(p), version=1)
            assert final_value(agg, ha) == reference_percentile(a, p)
            assert final_value(agg, ab) == reference_percentile(np.concatenate([a, b]), p)


def test_value_histogram_single_value_and_empty():
    one = ValueHistogram.from_values([42.5])
    empty = ValueHistogram()
    for p in PERCENTILES:
        agg = Aggregation("PERCENTILE", "c", percentile=float(p), version=1)
        assert final_value(agg, one) == 42.5
        assert final_value(agg, empty) == -math.inf  # DEFAULT_FINAL_RESULT
    assert merge_value("PERCENTILE", empty, one) == one == merge_value("PERCENTILE", one, empty)
    assert merge_value("PERCENTILE", empty, empty) == empty and empty.total == 0
    with pytest.raises(ValueError):
        final_value("PERCENTILE", one)  # the name alone carries no percentile


# ------------------------------------------------------------------ the reference's golden results, reduce level
@pytest.fixture(scope="module")
def percentile_spec():
    with open(os.path.join(GOLDEN, "sv_percentile_queries.json")) as f:
        return json.load(f)


def test_golden_file_shape(percentile_spec):
    cases = percentile_spec["cases"]
    assert len(cases) == 25
    assert sum("InterSegmentAggregationSingleValueQueriesTest" in c["source"] for c in cases) == 24
    for c in cases:
        assert set(c) == {"source", "sql", "rows", "delta", "stats"} and c["delta"] == 0 and len(c["stats"]) == 4
        assert re.search(r"\.java:\d+", c["source"])


def _group_histograms(keys, values):
    """{key: ValueHistogram of the key's values}."""
    order = np.lexsort((values, keys))
    k, v = keys[order], values[order]
    cuts = np.flatnonzero(k[1:] != k[:-1]) + 1
    out = {}
    for s, e in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [len(k)]])):
        if e > s:
            out[k[s].item()] = ValueHistogram.from_values(v[s:e])
    return out


def test_golden_cases_reduce_level(percentile_spec):
    """Per-copy histograms built with numpy from the fixture segment's data (the test's FILTER as a numpy mask), merged
    over the 4 copies (2 servers x 2 segments) by merge_intermediate, finished by final_result_table."""
    data = np.load(os.path.join(GOLDEN, "test_data_sv.npz"))
    d = {k: data[k] for k in data.files}
    mask = ((d["column1"] > 100000000) & (d["column3"] >= 20000000) & (d["column3"] <= 1000000000) &
            (d["column5"] == "gFuH") & ((d["column6"] < 500000000) | ~np.isin(d["column11"], ["t", "P"])) &
            (d["daysSinceEpoch"] == 126164076))
    assert int(mask.sum()) * 4 == 24516  # numDocsScanned of the filtered golden cases
    everything = np.ones(len(mask), dtype=bool)
    cache = {}

    def per_copy(column, group_by, filtered):
        key = (column, group_by, filtered)
        if key not in cache:
            m = mask if filtered else everything
            if group_by is None:
                cache[key] = ValueHistogram.from_values(d[column][m])
            else:
                cache[key] = _group_histograms(d[group_by][m], d[column][m].astype(np.float64))
        return cache[key]

    for case in percentile_spec["cases"]:
        q = parse_sql(case["sql"])
        filtered = q.filter is not None
        copy = IntermediateResult(list(q.aggregations), list(q.group_by))
        if q.group_by:
            hs = [per_copy(a.column, q.group_by[0], filtered) for a in q.aggregations]
            copy.groups = {(k,): [h[k] for h in hs] for k in hs[0]}
        else:
            copy.row = [per_copy(a.column, None, filtered) for a in q.aggregations]
        servers = [server_trim(merge_intermediate([copy, copy]), q) for _ in range(2)]
        got = final_result_table(merge_intermediate(servers), q)
        assert rows_match(got, case["rows"], case["delta"]), (case["source"], got, case["rows"])


# ------------------------------------------------------------------ C-ABI declarations
def test_parallel_tables():
    import torch
    from pinot_amd import parallel
    assert parallel.SECTION_OP[L.PA_ACC_HIST_U64] == torch.distributed.ReduceOp.SUM
    assert parallel.SECTION_DTYPE[L.PA_ACC_HIST_U64] == torch.int64


def test_abi_declarations():
    assert L.ABI_VERSION == 5
    assert L.PA_AGG_VALUE_HISTOGRAM == 7 and L.PA_ACC_HIST_U64 == 10
    header = open(os.path.join(ROOT, "include", "pinot_amd.h")).read()
    assert re.search(r"#define PA_ABI_VERSION 5\b", header)
    assert re.search(r"#define PA_AGG_VALUE_HISTOGRAM 7\b", header) and re.search(r"#define PA_ACC_HIST_U64 10\b", header)
    assert re.search(r"int64_t pa_query_fetch_histogram\(pa_query\* q, void\* stream, int32_t agg, int64_t num_groups, "
                     r"int64_t capacity,\s+int64_t\* out_row_ends, int32_t\* out_value_ids, "
                     r"int64_t\* out_value_counts\);", header)
    assert re.search(r"int pa_query_percentiles\(pa_query\* q, void\* stream, int32_t agg, int64_t num_groups, "
                     r"int32_t num_percentiles,\s+const double\* percentiles, int32_t\* out_value_ids\);", header)
    assert {"pa_query_fetch_histogram", "pa_query_percentiles"} <= set(L.EXPORTED)
