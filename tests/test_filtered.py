"""Filtered aggregations (AGG(x) FILTER (WHERE f)) without a GPU: the parser, the result column names (pinned by the two
strings FilteredAggregationsTest.java:219 and :226 spell out), the two references of tests/filtered_ref.py against each
other on the golden segment and on synthetic segments, the per-segment lane structure, and the reduce layer."""
import dataclasses

import numpy as np
import pytest

import filtered_ref as R
from pinot_amd import filter_stats as FS
from pinot_amd import parse_sql
from pinot_amd import query as Q
from pinot_amd import reduce as RD
from pinot_amd.segment import create_segment

SCHEMA = {"g": "INT", "h": "INT", "f1": "INT", "f2": "INT", "r": "INT", "x": "INT", "y": "LONG", "d": "DOUBLE",
          "s": "STRING"}
UNIVERSE = {"g": np.arange(20) * 3, "h": np.arange(3), "f1": np.arange(10), "f2": np.arange(8),
            "x": np.arange(50) - 7, "y": (np.arange(30, dtype=np.int64) - 4) * (1 << 33) + 5,
            "d": np.arange(40) * 0.37 - 3.0, "s": np.array(["a", "bb", "c", "dd", "e"])}


def make_segment(name, n, seed, full=False):
    """n docs of random draws from UNIVERSE; full: every value of every dictionary column occurs (n >= 50), so such
    segments share their dictionaries; otherwise the dictionaries are the segment's own (group and value remaps)."""
    rng = np.random.default_rng(seed)
    data = {}
    for c, u in UNIVERSE.items():
        v = u[rng.integers(0, len(u), size=n)]
        if full:
            assert n >= len(u)
            v[:len(u)] = u
        data[c] = v.astype({"INT": np.int32, "LONG": np.int64, "DOUBLE": np.float64}.get(SCHEMA[c], object))
    data["r"] = rng.integers(0, 100, size=n).astype(np.int32)
    return create_segment(name, data, SCHEMA, no_dictionary_columns=["r"])


def make_table(n):
    return [make_segment("own_%d" % n, n, 11 + n), make_segment("shared_a_%d" % n, max(n, 50), 5, full=True),
            make_segment("shared_b_%d" % n, max(n, 50) + 1, 6, full=True)]


# one query per shape the kernel treats differently (tests/test_gpu_filtered.py runs the same list on the GPU)
CASES = {
    "clause_only": "SELECT g, SUM(x) FILTER (WHERE f1 = 3), SUM(x) FILTER (WHERE f1 IN (1, 2, 5)), COUNT(*) FROM t "
                   "GROUP BY g LIMIT 1000",
    "clause_and_where_same_column": "SELECT g, SUM(x) FILTER (WHERE f1 > 2), COUNT(*) FILTER (WHERE f1 > 2), MIN(x) "
                                    "FROM t WHERE f1 < 7 GROUP BY g LIMIT 1000",
    "own_column": "SELECT g, h, SUM(y) FILTER (WHERE f2 > 4), MIN(x) FILTER (WHERE f2 > 4), MAX(d) FILTER (WHERE f2 <= 1), "
                  "SUM(d) FROM t WHERE f1 <> 9 GROUP BY g, h LIMIT 1000",
    "raw_leaf_and_or": "SELECT g, COUNT(*) FILTER (WHERE r BETWEEN 10 AND 50), SUM(d) FILTER (WHERE r < 30 OR f1 = 2), "
                       "MAX(y) FILTER (WHERE r < 30 OR f1 = 2) FROM t GROUP BY g LIMIT 1000",
    "negated_lanes": "SELECT g, SUM(x) FILTER (WHERE f1 <> 3), COUNT(*) FILTER (WHERE NOT f2 IN (1, 2)), MIN(d) FILTER "
                     "(WHERE f1 NOT IN (0, 4)) FROM t GROUP BY g LIMIT 1000",
    "negated_lanes_where": "SELECT g, SUM(x) FILTER (WHERE f1 <> 3), COUNT(*) FILTER (WHERE NOT f2 IN (1, 2)), COUNT(*) "
                           "FROM t WHERE f2 <> 7 GROUP BY g LIMIT 1000",
    "avg_pairs": "SELECT h, AVG(x), AVG(x) FILTER (WHERE f1 < 4), AVG(d) FILTER (WHERE f2 = 2), MINMAXRANGE(x) FILTER "
                 "(WHERE f2 = 2) FROM t GROUP BY h LIMIT 1000",
    "sets_and_hll": "SELECT h, DISTINCTCOUNTHLL(x) FILTER (WHERE f1 < 5), DISTINCTCOUNT(x) FILTER (WHERE f1 >= 5), "
                    "DISTINCTCOUNTHLL(s) FILTER (WHERE f2 IN (0, 3)), DISTINCTCOUNT(x) FROM t GROUP BY h LIMIT 1000",
    "empty_full_shared": "SELECT g, SUM(x) FILTER (WHERE f1 = 999), SUM(x) FILTER (WHERE r >= 0), SUM(x) FILTER (WHERE f1 "
                         ">= 0), COUNT(*) FILTER (WHERE f2 = 1), MAX(x) FILTER (WHERE f2 = 1), MIN(x) FILTER (WHERE f1 = 999) "
                         "FROM t WHERE f2 < 6 GROUP BY g LIMIT 1000",
    "no_main_lane": "SELECT g, SUM(x) FILTER (WHERE f1 = 3), MAX(x) FILTER (WHERE f2 = 1), AVG(x) FILTER (WHERE f2 = 1) "
                    "FROM t GROUP BY g LIMIT 1000",
    "no_main_lane_plus_count": "SELECT g, SUM(x) FILTER (WHERE f1 = 3), MAX(x) FILTER (WHERE f2 = 1), AVG(x) FILTER (WHERE "
                               "f2 = 1), COUNT(*) FROM t GROUP BY g LIMIT 1000",
    "aggregation_only": "SELECT SUM(x) FILTER (WHERE f1 = 3), COUNT(*) FILTER (WHERE f1 = 3), MIN(y) FILTER (WHERE f2 > 5), "
                        "AVG(d) FILTER (WHERE f2 > 5), COUNT(*), MAX(d) FROM t WHERE f1 <> 0",
    "aggregation_only_no_where": "SELECT SUM(y) FILTER (WHERE f1 < 3), COUNT(*) FILTER (WHERE r > 50) FROM t",
    "hot_key": "SELECT s, SUM(x) FILTER (WHERE f1 < 8), SUM(y) FILTER (WHERE f1 < 8), MIN(d) FILTER (WHERE f1 >= 1), "
               "COUNT(*) FROM t WHERE s = 'a' GROUP BY s LIMIT 1000",
}
DOUBLE_COLUMNS = ("d",)


# ------------------------------------------------------------------ parser and names
def test_parser_round_trip():
    q = parse_sql("SELECT SUM(a) FILTER (WHERE b = 1 AND c IN (2, 3)), COUNT(*) FILTER(WHERE NOT b > 4) AS n, "
                  "PERCENTILE95(a) FILTER (WHERE b < 2), PERCENTILE(a, 50) FILTER (WHERE b < 2), MAX(a) FROM t "
                  "WHERE c <> 9 GROUP BY c ORDER BY SUM(a) FILTER (WHERE b = 1 AND c IN (2, 3)) DESC, MAX(a) LIMIT 5")
    a = q.aggregations
    assert a[0] == Q.Aggregation("SUM", "a", filter=Q.And((Q.EqPredicate("b", "1"), Q.InPredicate("c", ("2", "3")))))
    assert a[1] == Q.Aggregation("COUNT", filter=Q.Not(Q.RangePredicate("b", "4", False)))
    assert a[2].function == "PERCENTILE" and a[2].percentile == 95.0 and a[2].filter == Q.RangePredicate(
        "b", Q.UNBOUNDED, False, "2", False)
    assert a[3].version == 1 and a[3].filter == a[2].filter
    assert a[4].filter is None and q.aliases[1] == "n"
    assert q.order_by[0].expr == a[0] and q.order_by[1].expr == a[4] and len(a) == 5
    assert q.columns() == {"a", "b", "c"} and Q.query_columns(q) == ["c", "a", "b"]
    # the same function under another filter is another aggregation; ORDER BY on it adds it
    q = parse_sql("SELECT SUM(a) FILTER (WHERE b = 1) FROM t GROUP BY c ORDER BY SUM(a) FILTER (WHERE b = 2)")
    assert len(q.aggregations) == 2 and q.num_select_aggs == 1
    assert q.aggregations[0] != q.aggregations[1] != dataclasses.replace(q.aggregations[1], filter=None)


@pytest.mark.parametrize("sql", [
    "SELECT SUM(a) FILTER (b = 1) FROM t",               # no WHERE
    "SELECT SUM(a) FILTER WHERE b = 1 FROM t",            # no parentheses
    "SELECT SUM(a) FILTER (WHERE b = 1 FROM t",           # not closed
    "SELECT SUM(a) FILTER (WHERE) FROM t",                # no filter
    "SELECT a FILTER (WHERE b = 1) FROM t",               # not an aggregation
    "SELECT DISTINCT a FILTER (WHERE b = 1) FROM t",
])
def test_parser_rejections(sql):
    # (the FILTER grammar's own message: a parser without it refuses these too, at the word FILTER)
    with pytest.raises(ValueError, match="^FILTER clause: "):
        parse_sql(sql)


def test_result_names():
    # FilteredAggregationsTest.java:219 and :226
    q = parse_sql("SELECT SUM(INT_COL) FILTER(WHERE INT_COL > 9999) FROM MyTable WHERE INT_COL < 1000000 GROUP BY "
                  "BOOLEAN_COL")
    assert q.aggregations[0].result_name == "sum(INT_COL) FILTER(WHERE INT_COL > '9999')"
    q = parse_sql("SELECT SUM(INT_COL) FILTER(WHERE INT_COL > 9999 AND INT_COL < 1000000) FROM MyTable GROUP BY "
                  "BOOLEAN_COL")
    assert q.aggregations[0].result_name == "sum(INT_COL) FILTER(WHERE (INT_COL > '9999' AND INT_COL < '1000000'))"
    names = [a.result_name for a in parse_sql(
        "SELECT COUNT(*) FILTER (WHERE a = 'x'), MIN(m) FILTER (WHERE a != 3), MAX(m) FILTER (WHERE a IN (1, 2)), "
        "AVG(m) FILTER (WHERE a NOT IN ('p', 'q')), SUM(m) FILTER (WHERE a BETWEEN 1 AND 2), SUM(m) FILTER (WHERE a >= 1 "
        "OR NOT b <= 2), SUM(m) FILTER (WHERE a > 1 AND (b < 2 OR c = 3)), DISTINCTCOUNTHLL(m, 12) FILTER (WHERE TRUE), "
        "PERCENTILE(m, 99.9) FILTER (WHERE a = 1), COUNT(*) FROM t").aggregations]
    assert names == [
        "count(*) FILTER(WHERE a = 'x')", "min(m) FILTER(WHERE a != '3')", "max(m) FILTER(WHERE a IN ('1','2'))",
        "avg(m) FILTER(WHERE a NOT IN ('p','q'))", "sum(m) FILTER(WHERE a BETWEEN '1' AND '2')",
        "sum(m) FILTER(WHERE (a >= '1' OR (NOT b <= '2')))", "sum(m) FILTER(WHERE (a > '1' AND (b < '2' OR c = '3')))",
        "distinctcounthll(m) FILTER(WHERE true)", "percentile(m, 99.9) FILTER(WHERE a = '1')", "count(*)"]


# ------------------------------------------------------------------ the references against each other
GOLDEN_CASES = {
    # one query per shape class of FilteredAggregationsTest.java, on this project's golden segment
    "filter_only_in_clause (:177-179)":
        "SELECT SUM(column1) FILTER (WHERE column6 > 319376192) FROM testTable",
    "clause_plus_where (:165-167)":
        "SELECT SUM(column1) FILTER (WHERE column6 > 319376192), COUNT(*) FILTER (WHERE column6 > 319376192) FROM testTable "
        "WHERE column7 < 1985159279",
    "several_clauses_plus_unfiltered (:379-391)":
        "SELECT MIN(column3) FILTER (WHERE column11 = 'P'), MAX(column3) FILTER (WHERE column11 = 'P'), SUM(column1) "
        "FILTER (WHERE column17 IN (83386499, 227908817, 1284373442)), SUM(column3), COUNT(*) FROM testTable WHERE column12 <> 'zz'",
    "min_max_avg (:189-198)":
        "SELECT MIN(column1) FILTER (WHERE column9 > 296467636), MAX(column1) FILTER (WHERE column9 <= 296467636), AVG(column3) "
        "FILTER (WHERE column9 > 296467636), AVG(column3) FROM testTable",
    "group_by_order_by_filtered (:455-463)":
        "SELECT column11, SUM(column1) FILTER (WHERE column17 > 1284373442), COUNT(*) FROM testTable WHERE column6 > 296467636 GROUP BY "
        "column11 ORDER BY SUM(column1) FILTER (WHERE column17 > 1284373442) DESC LIMIT 3",
}


@pytest.mark.parametrize("name", sorted(GOLDEN_CASES))
def test_golden_references_agree(golden_segment, name):
    q = parse_sql(GOLDEN_CASES[name])
    a, b = R.compose(q, [golden_segment]), R.numpy_eval(q, [golden_segment])
    R.assert_same(a, b)
    assert a.num_docs_scanned > 0
    # the reference's test method: a filtered column is the unfiltered query with the filter moved into WHERE
    import oracle
    for i, agg in enumerate(q.aggregations):
        if agg.filter is None:
            continue
        plain = oracle.run_query(R.lane_query(q, agg.filter, [agg]), [golden_segment])
        if q.group_by:
            for k, row in plain.groups.items():
                assert R._same_value(agg.function, a.groups[k][i], row[0], 0.0)
        else:
            assert R._same_value(agg.function, a.row[i], plain.row[0], 0.0)


@pytest.fixture(scope="module")
def table():
    return make_table(2049)


@pytest.mark.parametrize("name", sorted(CASES))
def test_synthetic_references_agree(table, name):
    q = parse_sql(CASES[name])
    R.assert_same(R.compose(q, table), R.numpy_eval(q, table), double_sum_columns=DOUBLE_COLUMNS)


def test_empty_values_and_missing_groups():
    """A group only one lane saw holds the other lanes' empty values; without an unfiltered aggregation a group no lane
    saw does not exist, and COUNT(*) brings it back (FilteredGroupByOperator.java:117-150)."""
    data = {c: np.zeros(4, dtype=np.int32) for c in SCHEMA}
    data["g"] = np.array([0, 0, 3, 6], dtype=np.int32)
    data["f1"] = np.array([1, 1, 2, 5], dtype=np.int32)
    data["x"] = np.array([10, 20, 30, 40], dtype=np.int32)
    data["y"] = data["y"].astype(np.int64)
    data["d"] = data["d"].astype(np.float64)
    data["s"] = np.array(["a"] * 4, dtype=object)
    seg = create_segment("tiny", data, SCHEMA, no_dictionary_columns=["r"])
    q = parse_sql("SELECT g, MIN(x) FILTER (WHERE f1 = 1), MAX(x) FILTER (WHERE f1 = 2), AVG(x) FILTER (WHERE f1 = 2) FROM t "
                  "GROUP BY g")
    for ref in (R.compose(q, [seg]), R.numpy_eval(q, [seg])):
        assert set(ref.groups) == {(0,), (3,)}
        assert ref.groups[(0,)][0] == 10.0 and ref.groups[(0,)][1] == float("-inf")
        assert ref.groups[(0,)][2].sum == 0.0 and ref.groups[(0,)][2].count == 0
        assert ref.groups[(3,)][0] == float("inf") and ref.groups[(3,)][1] == 30.0
    q2 = parse_sql("SELECT g, MIN(x) FILTER (WHERE f1 = 1), COUNT(*) FROM t GROUP BY g")
    assert set(R.compose(q2, [seg]).groups) == {(0,), (3,), (6,)}
    assert R.compose(q2, [seg]).groups[(6,)] == [float("inf"), 1]


def test_lane_structure_of_a_segment():
    """A sub filter that covers a segment's whole dictionary joins the main lane there, under a main filter that is not
    match-all (AggregationFunctionUtils.java:353-354, :376-378); equal filters share a lane; an empty main filter leaves
    one lane."""
    seg = make_segment("s", 200, 3, full=True)
    q = parse_sql("SELECT SUM(x) FILTER (WHERE f1 >= 0), SUM(y) FILTER (WHERE f1 = 3), MAX(d) FILTER (WHERE f1 = 3), "
                  "COUNT(*) FROM t WHERE f2 < 6 GROUP BY g")
    a = q.aggregations
    lanes = FS.lane_structure(q, seg)
    assert lanes == [(a[1].filter, [a[1], a[2]]), (None, [a[3], a[0]])]
    assert [(f, aggs) for f, aggs in R.segment_lanes(q, seg)] == lanes
    assert FS.lane_projected_columns(q, lanes[0][1]) == 3 and FS.lane_projected_columns(q, lanes[1][1]) == 2
    # under a match-all main filter the whole-dictionary sub filter keeps its own lane (:351-352)
    q2 = dataclasses.replace(q, filter=None)
    assert [f for f, _ in FS.lane_structure(q2, seg)] == [a[0].filter, a[1].filter, None]
    assert [f for f, _ in R.segment_lanes(q2, seg)] == [a[0].filter, a[1].filter, None]
    # an empty main filter: one lane, no docs (:321-329)
    q3 = dataclasses.replace(q, filter=parse_sql("SELECT COUNT(*) FROM t WHERE f2 = 99").filter)
    assert FS.lane_structure(q3, seg) == [("empty", list(a))] and R.segment_lanes(q3, seg) == []
    # the statistics count the joined lane once
    docs = int(R.SR.filter_mask(q.filter, seg).sum())
    sub = int(R.SR.filter_mask(Q.And((q.filter, a[1].filter)), seg).sum())
    ref = R.numpy_eval(q, [seg])
    assert ref.num_docs_scanned == docs + sub
    assert ref.num_entries_scanned_post_filter == docs * 2 + sub * 3


# ------------------------------------------------------------------ reduce
def test_reduce_merge_final_and_order_by(table):
    sql = ("SELECT g, SUM(x) FILTER (WHERE f1 < 5), AVG(x) FILTER (WHERE f2 = 1), COUNT(*) FILTER (WHERE f1 < 5), COUNT(*) "
           "FROM t WHERE f2 < 7 GROUP BY g ORDER BY SUM(x) FILTER (WHERE f1 < 5) DESC, g LIMIT 4")
    q = parse_sql(sql)
    whole = R.compose(q, table)
    parts = [R.compose(q, table[:1]), R.compose(q, table[1:])]
    merged = RD.merge_intermediate(parts)
    R.assert_same(merged, whole, stats=False)
    assert merged.num_docs_scanned == whole.num_docs_scanned
    assert merged.num_entries_scanned_post_filter == whole.num_entries_scanned_post_filter
    assert merged.num_entries_scanned_in_filter is None
    rows = RD.final_result_table(RD.server_trim(merged, q), q)
    assert len(rows) == 4 and [r[1] for r in rows] == sorted((r[1] for r in rows), reverse=True)
    full = sorted(((v[0], k[0]) for k, v in whole.groups.items()), key=lambda t: (-t[0], t[1]))[:4]
    assert [(r[1], r[0]) for r in rows] == full
    # the ORDER BY expression must carry its filter: the unfiltered SUM is not in the select list
    bad = dataclasses.replace(q, order_by=[Q.OrderBy(Q.Aggregation("SUM", "x"), False)])
    with pytest.raises(ValueError):
        RD.final_result_table(merged, bad)
