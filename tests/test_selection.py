"""Selection queries on the CPU: the parser, the numpy restatement (tests/selection_ref.py) against the reference's own
golden results (tests/golden/sv_selection.json, from InnerSegmentSelectionSingleValueQueriesTest.java), the broker merge
(reduce.merge_selection), the UTF-16 string order, the numEntriesScannedPostFilter formula and the gloo gather. The GPU
path is checked against the same restatement in tests/test_gpu_selection.py."""
import dataclasses
import json
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import oracle
import selection_ref as R
from conftest import GOLDEN
from pinot_amd import filter_stats as FS
from pinot_amd import parse_sql
from pinot_amd import query as Q
from pinot_amd import selection as S
from pinot_amd.reduce import merge_selection
from pinot_amd.segment import create_segment


@pytest.fixture(scope="module")
def selection_spec():
    with open(os.path.join(GOLDEN, "sv_selection.json")) as f:
        return json.load(f)


def case_sql(spec, case):
    return case["sql"].replace("{FILTER}", spec["filter"])


# ------------------------------------------------------------------ parser
def test_parse_select_star_and_limit_forms():
    q = parse_sql("SELECT * FROM testTable LIMIT 5000, 7000")
    assert q.is_selection and q.select_star and (q.offset, q.limit) == (5000, 7000) and not q.select_columns
    q = parse_sql("SELECT a, b FROM t WHERE a > 3 ORDER BY b DESC, a LIMIT 10 OFFSET 4")
    assert q.is_selection and not q.select_star and q.select_columns == ["a", "b"]
    assert (q.offset, q.limit) == (4, 10)
    assert q.order_by == [Q.OrderBy("b", False), Q.OrderBy("a", True)]
    q = parse_sql("SELECT a FROM t ORDER BY c")
    assert q.is_selection and q.offset == 0 and q.limit == 10 and q.columns() == {"a", "c"}
    assert parse_sql("SELECT * FROM t WHERE x = 1 LIMIT 0").limit == 0


def test_aggregation_queries_parse_as_before():
    q = parse_sql("SELECT COUNT(*), SUM(m) FROM t WHERE d = 3")
    assert not q.is_selection and q.offset == 0 and not q.select_star
    assert [a.function for a in q.aggregations] == ["COUNT", "SUM"] and q.columns() == {"m", "d"}
    q = parse_sql("SELECT d, SUM(m) FROM t GROUP BY d ORDER BY SUM(m) DESC LIMIT 7")
    assert not q.is_selection and q.select_columns == ["d"] and q.group_by == ["d"] and q.limit == 7 and q.offset == 0
    assert q.columns() == {"d", "m"}
    with pytest.raises(ValueError):
        parse_sql("SELECT d, SUM(m) FROM t")  # plain column next to an aggregation without GROUP BY
    with pytest.raises(ValueError):
        parse_sql("SELECT *, COUNT(*) FROM t")


# ------------------------------------------------------------------ golden cases through the restatement
def check_golden_case(case, res, query, stats):
    """One golden case against a server result: row count, schema, the asserted row, the statistics where modelled.
    res: columns, rows (in `columns` order); stats: [docs, in filter, post filter, total] of the result."""
    assert len(res.rows) == case["num_rows"], case["source"]
    assert len(res.columns) == case["num_columns"], case["source"]
    if "schema" in case:
        assert list(res.columns) == case["schema"], case["source"]
    if "row" in case:
        row = res.rows[case["row"]]
        assert len(row) == case["num_columns"]
        for name, v in case["values"].items():
            assert row[res.columns.index(name)] == v, (case["source"], name)
    if case["stats"] is not None:
        assert stats == case["stats"], case["source"]


def test_reference_restatement_reproduces_golden_cases(selection_spec, golden_segment):
    from test_filter_stats import leaf_masks
    seg = golden_segment
    for case in selection_spec["cases"]:
        q = parse_sql(case_sql(selection_spec, case))
        res = R.run(q, [seg])
        types = [seg.column(c).data_type for c in res.columns]
        for name, t in case.get("types", {}).items():
            assert types[res.columns.index(name)] == t
        if "schema_types" in case:
            assert types == case["schema_types"]
        stats = None
        if case["stats"] is not None:
            if q.limit + q.offset == 0:
                stats = [0, 0, 0, seg.num_docs]
            else:
                count = dataclasses.replace(q, aggregations=[Q.Aggregation("COUNT")], aliases=[None], order_by=[],
                                            select_columns=[], select_star=False, num_select_aggs=1)
                masks = leaf_masks(count, seg)
                in_filter = FS.server_stats(count, [seg], lambda si: masks)[0] if q.filter is not None else 0
                stats = [res.matched, in_filter, R.post_filter_entries(q, res), seg.num_docs]
        check_golden_case(case, res, q, stats)
        # the broker's view: offset dropped
        names, rows = R.broker_rows(q, res)
        assert len(rows) == max(0, min(case["num_rows"] - q.offset, q.limit))


def test_reference_filter_matches_the_oracle(selection_spec, golden_segment):
    """The restatement's match mask against the pinned oracle's COUNT(*) for the same WHERE."""
    wheres = [selection_spec["filter"], " WHERE column6 < 500000000 OR column11 NOT IN ('t', 'P')",
              " WHERE column1 > 100000000 AND NOT column3 BETWEEN 20000000 AND 1000000000", " WHERE column5 != 'gFuH'"]
    for w in wheres:
        q = parse_sql("SELECT COUNT(*) FROM testTable" + w)
        assert int(R.filter_mask(q.filter, golden_segment).sum()) == oracle.run_query(q, [golden_segment]).row[0], w
    assert int(R.filter_mask(parse_sql("SELECT COUNT(*) FROM t" + wheres[0]).filter, golden_segment).sum()) == 6129


# ------------------------------------------------------------------ orders
def test_utf16_order_differs_from_code_point_order():
    """String.compareTo compares UTF-16 code units: U+FFFF (one unit 0xFFFF) sorts AFTER U+10000 (units 0xD800 0xDC00),
    the opposite of the code-point order numpy and Python use."""
    lo, hi = "\U00010000", "\uffff"
    assert sorted([hi, lo]) == [hi, lo]  # code points: U+FFFF < U+10000
    assert sorted([hi, lo], key=S.utf16_key) == [lo, hi]
    vals, keys = S.table_order_dictionary([np.array(["b", hi, "a"]), np.array([lo, "a"])], "STRING")
    assert vals.tolist() == ["a", "b", lo, hi]
    assert S.order_remap(keys, np.array(["a", lo, hi]), "STRING").tolist() == [0, 2, 3]
    assert R.value_ranks(np.array([hi, lo, "a"]), "STRING").tolist() == [2, 1, 0]
    # and through the restatement: a segment ordered by such a column
    seg = create_segment("u", {"s": np.array([hi, "a", lo, "b"]), "i": np.arange(4, dtype=np.int32)},
                         {"s": "STRING", "i": "INT"})
    assert [r[0] for r in R.run(parse_sql("SELECT s FROM t ORDER BY s"), [seg]).rows] == ["a", "b", lo, hi]
    assert [r[0] for r in R.run(parse_sql("SELECT s FROM t ORDER BY s DESC"), [seg]).rows] == [hi, lo, "b", "a"]


def test_double_compare_order():
    nan = float("nan")
    v = np.array([0.0, -0.0, nan, float("inf"), -float("inf"), 1.5, -1.5])
    order = np.argsort(S.float_order_bits(v), kind="stable")
    assert [repr(float(x)) for x in v[order]] == ["-inf", "-1.5", "-0.0", "0.0", "1.5", "inf", "nan"]
    assert R.value_ranks(v, "DOUBLE").tolist() == [3, 2, 6, 5, 0, 4, 1]
    bits = S.float_order_bits(np.array([nan, -nan]))
    assert bits[0] == bits[1]  # every NaN is one value


# ------------------------------------------------------------------ statistics formula
def test_post_filter_entries_formula():
    # every output column ordered: matched x projected columns
    assert S.post_filter_entries([100, 50], 10, 2, 0) == 300
    # otherwise: matched x order-by columns + sum over segments of min(K, matched) x other columns
    assert S.post_filter_entries([30000], 10, 2, 2) == 60020           # testSelectionOrderBy
    assert S.post_filter_entries([6129], 12000, 2, 9) == 67419         # testSelectStarOrderByLargeOffsetLimit, filtered
    assert S.post_filter_entries([100, 3, 0], 10, 1, 4) == 103 + (10 + 3 + 0) * 4


# ------------------------------------------------------------------ broker merge
def _result(cols, types, rows):
    return S.SelectionResult(list(cols), list(types), rows=[list(r) for r in rows])


def test_merge_selection_offset_limit_ties_and_projection():
    q = parse_sql("SELECT name, v FROM t ORDER BY v DESC, k LIMIT 2, 3")
    cols, types = ["v", "k", "name"], ["INT", "INT", "STRING"]
    a = _result(cols, types, [[9, 1, "a0"], [7, 5, "a1"], [7, 6, "a2"], [1, 0, "a3"]])
    b = _result(cols, types, [[9, 1, "b0"], [8, 2, "b1"], [7, 5, "b2"]])
    names, rows = merge_selection([a, b], q)
    assert names == ["name", "v"]
    # merged: (9,1,a0) (9,1,b0) | (8,2,b1) (7,5,a1) (7,5,b2) | (7,6,a2) (1,0,a3): ties keep server order
    assert rows == [["b1", 8], ["a1", 7], ["b2", 7]]
    names, rows = merge_selection([b, a], q)
    assert rows == [["b1", 8], ["b2", 7], ["a1", 7]]
    # no ORDER BY: server order, then offset / limit
    q2 = parse_sql("SELECT v FROM t LIMIT 1, 4")
    names, rows = merge_selection([_result(["v"], ["INT"], [[1], [2]]), _result(["v"], ["INT"], [[3], [4], [5]])], q2)
    assert (names, rows) == (["v"], [[2], [3], [4], [5]])
    # SELECT *: the columns by name
    q3 = parse_sql("SELECT * FROM t ORDER BY v LIMIT 1")
    names, rows = merge_selection([_result(["v", "a", "z"], ["INT", "INT", "INT"], [[1, 2, 3]])], q3)
    assert (names, rows) == (["a", "v", "z"], [[2, 1, 3]])


def test_merge_selection_equals_one_server_over_all_segments():
    """Two servers' results merged = the restatement over both servers' segments (server order = segment order)."""
    from synth import make_segment
    cols = {"a": ("INT", 7), "s": ("STRING", 5), "d": ("DOUBLE", 40)}
    segs = [make_segment(70 + i, 300 + 50 * i, cols) for i in range(4)]
    for sql in ("SELECT s, d FROM t WHERE a > -100000000 ORDER BY a, s DESC LIMIT 3, 20",
                "SELECT * FROM t ORDER BY s DESC, d LIMIT 15", "SELECT d FROM t LIMIT 2, 9"):
        q = parse_sql(sql)
        parts = []
        for half in (segs[:2], segs[2:]):
            r = R.run(q, half)
            parts.append(S.SelectionResult(r.columns, [half[0].column(c).data_type for c in r.columns], rows=r.rows))
        names, rows = merge_selection(parts, q)
        if not q.order_by:  # every server keeps its first K docs; the broker takes them in server order
            exp = R.broker_rows(q, R.run(q, segs[:2]))
        else:
            exp = R.broker_rows(q, R.run(q, segs))
        assert (names, rows) == exp, sql


# ------------------------------------------------------------------ gloo gather
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_result(rank):
    rows = [[5, "r%d" % rank], [7, "r%d" % rank]] if rank == 0 else [[5, "r1"], [6, "r1"]]
    return S.SelectionResult(["v", "name"], ["INT", "STRING"], rows=rows)


def _gather_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from pinot_amd.parallel import gather_selection
    q = parse_sql("SELECT name, v FROM t ORDER BY v LIMIT 1, 2")
    out[rank] = gather_selection(_rank_result(rank), q)
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_gather_selection():
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_gather_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    # merged: (5, r0) (5, r1) (6, r1) (7, r0); offset 1, limit 2
    assert out[0] == out[1] == (["name", "v"], [["r1", 5], ["r1", 6]])
