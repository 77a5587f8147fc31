"""Distinct queries without a GPU: the parser, the restatement tests/distinct_ref.py against the reference's golden
cases (tests/golden/sv_distinct.json), the broker merge reduce.merge_distinct against the restatement's reducer, and the
completed comparator against numpy.lexsort."""
import json
import os

import numpy as np
import pytest

import distinct_ref as R
from conftest import GOLDEN
from pinot_amd import parse_sql
from pinot_amd.segment import create_segment


def golden():
    with open(os.path.join(GOLDEN, "sv_distinct.json")) as f:
        return json.load(f)


def distinct_queries_table(spec):
    """DistinctQueriesTest's two segments (:159-160, :180-217) as dictionary columns."""
    t = spec["distinct_queries"]["table"]
    u, n = t["num_unique_records_per_segment"], t["num_records_per_segment"]
    segs = []
    for i, base in enumerate(t["bases"]):
        v = np.tile(np.arange(base, base + u), n // u)
        data = {"intColumn": v.astype(np.int32), "longColumn": v.astype(np.int64), "floatColumn": v.astype(np.float32),
                "doubleColumn": v.astype(np.float64), "stringColumn": np.array([str(x) for x in v.tolist()])}
        segs.append(create_segment("testTable_%d" % i, data, t["schema"]))
    return segs


def as_set(rows):
    return {int(r[0]) if not isinstance(r[0], str) else r[0] for r in rows}


# ------------------------------------------------------------------ parser
def test_parser_spellings_and_columns():
    q = parse_sql("SELECT DISTINCT column1 FROM testTable")
    assert q.is_distinct and not q.is_selection and not q.aggregations and not q.group_by
    assert q.select_columns == ["column1"] and q.limit == 10 and q.order_by == []
    q = parse_sql("SELECT DISTINCT(column1) FROM testTable LIMIT 1000000")
    assert q.is_distinct and q.select_columns == ["column1"] and q.limit == 1000000
    q = parse_sql("SELECT DISTINCT a, b, c FROM t WHERE d > 3 AND a IN (1, 2) ORDER BY c DESC, a ASC LIMIT 7")
    assert q.is_distinct and not q.is_selection
    assert q.select_columns == ["a", "b", "c"]
    assert [(o.expr, o.asc) for o in q.order_by] == [("c", False), ("a", True)]
    assert q.limit == 7 and q.filter is not None
    assert q.columns() == {"a", "b", "c", "d"}
    q = parse_sql("SELECT DISTINCT a, b FROM t LIMIT 3, 5")
    assert (q.offset, q.limit) == (3, 5)
    q = parse_sql("SELECT DISTINCT a FROM t LIMIT 5 OFFSET 2")
    assert (q.offset, q.limit) == (2, 5)
    # the other families keep their flags
    assert parse_sql("SELECT a FROM t").is_selection and not parse_sql("SELECT a FROM t").is_distinct
    g = parse_sql("SELECT a, COUNT(*) FROM t GROUP BY a")
    assert not g.is_distinct and not g.is_selection
    assert parse_sql("SELECT COUNT(DISTINCT a) FROM t").aggregations[0].function == "DISTINCTCOUNT"


@pytest.mark.parametrize("sql", [
    "SELECT DISTINCT a FROM t ORDER BY b",
    "SELECT DISTINCT a, b FROM t ORDER BY a, c DESC",
    "SELECT DISTINCT a, SUM(b) FROM t",
    "SELECT DISTINCT(a), COUNT(*) FROM t",
    "SELECT DISTINCT SUM(b) FROM t",
    "SELECT DISTINCT(a, b) FROM t",
])
def test_parser_refusals(sql):
    with pytest.raises(ValueError):
        parse_sql(sql)


# ------------------------------------------------------------------ the restatement on the golden cases
def test_restatement_inner_segment_golden(golden_segment):
    for case in golden()["inner_segment"]:
        q = parse_sql(case["sql"])
        assert list(q.select_columns) == case["columns"]
        types = R.column_types(q, [golden_segment])
        assert types == case["types"]
        assert R.uses_dictionary_operator(q, golden_segment) == (case["operator"] == "DictionaryBasedDistinctOperator")
        recs, stats = R.reference_server(q, [golden_segment])
        assert len(recs) == case["size"], case["source"]
        vals = np.stack([R.SR.decoded(golden_segment, c) for c in q.select_columns], axis=1)
        uniq = np.unique(vals, axis=0)
        assert len(uniq) == case["size"]
        assert sorted(tuple(r) for r in recs) == [tuple(r) for r in uniq.tolist()]
        if case["operator"] == "DictionaryBasedDistinctOperator":
            assert stats == {"numDocsScanned": case["size"], "numEntriesScannedPostFilter": case["size"],
                             "numTotalDocs": golden_segment.num_docs}
        else:
            assert stats["numDocsScanned"] == golden_segment.num_docs
            assert stats["numEntriesScannedPostFilter"] == 2 * golden_segment.num_docs
        done = R.completed_server(q, [golden_segment])
        assert done.present == case["size"]
        assert sorted(tuple(r) for r in done.rows) == [tuple(r) for r in uniq.tolist()]


def test_restatement_distinct_queries_golden():
    spec = golden()
    segs = distinct_queries_table(spec)
    for case in spec["distinct_queries"]["cases"]:
        q = parse_sql(case["sql"])
        used = [segs[i] for i in case["segments"]]
        types = R.column_types(q, used)
        if case.get("broker"):
            # (each segment is its own server table here; the broker merges them)
            tables = [R.reference_server(q, [s])[0] for s in used]
            rows = R.reference_broker(q, tables, types)
            assert rows == case["rows"], case["source"]
            assert R.completed_broker(q, [R.completed_server(q, [s]).rows for s in used], types) == case["rows"]
            continue
        recs, _ = R.reference_server(q, used)
        assert len(recs) == len(case["set"]), case["source"]
        assert as_set(recs) == set(case["set"]), case["source"]
        # the deterministic completion returns the same set on every golden case (and sorted)
        done = R.completed_server(q, used)
        assert as_set(done.rows) == set(case["set"]), case["source"]


# ------------------------------------------------------------------ the completed comparator
def _random_records(rng, n):
    strs = np.array(["a", "b", "\uffff", "\U00010000", "zz", ""])
    return [[int(rng.integers(0, 5)), float(rng.integers(-3, 3)) / 2, str(strs[rng.integers(0, len(strs))])]
            for _ in range(n)]


@pytest.mark.parametrize("order", ["", "ORDER BY b", "ORDER BY c DESC", "ORDER BY b DESC, a", "ORDER BY c, b DESC, a DESC"])
def test_completed_comparator_is_lexsort(order):
    from pinot_amd import distinct as D
    rng = np.random.default_rng(5)
    types = ["INT", "DOUBLE", "STRING"]
    q = parse_sql("SELECT DISTINCT a, b, c FROM t %s LIMIT 1000" % order)
    recs = R.unique_records(_random_records(rng, 400), types)
    got = D.sort_records(recs, types, D.completed_order(q))
    # numpy.lexsort with the documented completion: ORDER BY entries, then the unnamed columns ascending, select order
    entries = R.completed_entries(q)
    named = [q.select_columns.index(o.expr) for o in q.order_by]
    assert [j for j, _ in entries] == named + [j for j in range(3) if j not in named]
    assert all(asc for j, asc in entries if j not in named)
    assert D.completed_order(q) == entries
    ranks = np.stack([R.SR.value_ranks(np.array([r[j] for r in recs], dtype=object if t == "STRING" else None), t)
                      for j, t in enumerate(types)], axis=1)
    keys = [ranks[:, j] if asc else -ranks[:, j] for j, asc in reversed(entries)]
    assert got == [recs[i] for i in np.lexsort(keys).tolist()]
    # UTF-16 order: the supplementary-plane character sorts below U+FFFF
    col_c = [r[2] for r in D.sort_records(recs, types, [(2, True), (0, True), (1, True)])]
    assert col_c.index("\U00010000") < col_c.index("\uffff")


# ------------------------------------------------------------------ the broker merge
def _result(rows, types, cols=("a", "b")):
    from pinot_amd.distinct import DistinctResult
    return DistinctResult(list(cols), list(types), rows=[list(r) for r in rows], present=len(rows))


@pytest.mark.parametrize("sql,parts", [
    # duplicates across partials
    ("SELECT DISTINCT a, b FROM t LIMIT 10", [[[1, 1], [2, 2]], [[2, 2], [1, 1], [0, 5]], [[0, 5]]]),
    # a cut inside a tie class: ORDER BY a alone, three records with a = 1, the limit falls among them
    ("SELECT DISTINCT a, b FROM t ORDER BY a LIMIT 3", [[[0, 9], [1, 7], [1, 3]], [[1, 5], [1, 3], [2, 0]]]),
    ("SELECT DISTINCT a, b FROM t ORDER BY a DESC LIMIT 2", [[[2, 4], [2, 1]], [[2, 3], [2, 1]], [[2, 9]]]),
    # limit larger than the union
    ("SELECT DISTINCT a, b FROM t ORDER BY b DESC, a LIMIT 100", [[[1, 1], [2, 2]], [[3, 3]], []]),
    ("SELECT DISTINCT a, b FROM t LIMIT 100", [[[5, 1]], [[4, 2], [5, 1]]]),
])
def test_merge_distinct_equals_reducer(sql, parts):
    from pinot_amd.reduce import merge_distinct
    q = parse_sql(sql)
    types = ["INT", "INT"]
    cols, rows = merge_distinct([_result(p, types) for p in parts], q)
    assert cols == ["a", "b"]
    expect = R.completed_broker(q, parts, types)
    assert rows == expect
    assert len(rows) == min(q.limit, len(R.unique_records([r for p in parts for r in p], types)))
    # against the reference's reducer: the ORDER BY columns of every row agree position by position (the tie class at the
    # cut is the reference's to choose), and without ORDER BY the sizes agree
    ref = R.reference_broker(q, parts, types)
    assert len(ref) == len(rows)
    idx = [j for j, _ in R.order_entries(q)]
    assert [[r[j] for j in idx] for r in ref] == [[r[j] for j in idx] for r in rows]


def test_merge_distinct_ignores_offset_and_checks_columns():
    from pinot_amd.reduce import merge_distinct
    q = parse_sql("SELECT DISTINCT a, b FROM t ORDER BY a LIMIT 1, 2")
    _, rows = merge_distinct([_result([[1, 1], [2, 2], [3, 3]], ["INT", "INT"])], q)
    assert rows == [[1, 1], [2, 2]]  # DistinctDataTableReducer.java:56: the limit alone
    with pytest.raises(ValueError):
        merge_distinct([_result([[1, 1]], ["INT", "INT"]), _result([[1, 1]], ["INT", "INT"], cols=("b", "a"))], q)


def test_dictionary_fast_path_rows_and_statistics():
    from pinot_amd import distinct as D
    spec = golden()
    segs = distinct_queries_table(spec)
    for sql in ("SELECT DISTINCT(intColumn) FROM testTable", "SELECT DISTINCT(stringColumn) FROM testTable ORDER BY stringColumn DESC LIMIT 150",
                "SELECT DISTINCT(floatColumn) FROM testTable ORDER BY floatColumn DESC LIMIT 7"):
        q = parse_sql(sql)
        assert D.dictionary_fast_path(q, segs)
        got = D.dictionary_distinct(q, segs)
        ref = R.completed_server(q, segs)
        assert ref.fast_path and got.rows == ref.rows and got.present == ref.present == 200
        assert (got.num_docs_scanned, got.num_entries_scanned_in_filter, got.num_entries_scanned_post_filter,
                got.num_total_docs) == (ref.matched, 0, ref.post, 20000)
    assert not D.dictionary_fast_path(parse_sql("SELECT DISTINCT intColumn FROM t WHERE floatColumn > 2"), segs)
    assert not D.dictionary_fast_path(parse_sql("SELECT DISTINCT intColumn, longColumn FROM t"), segs)
