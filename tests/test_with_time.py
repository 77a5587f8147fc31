"""FIRSTWITHTIME / LASTWITHTIME on the host (no GPU): the parser and the result column names, the plain-Python
restatement against a brute-force sort, the broker's merge and final values, the Java casts of the declared type, the
C-ABI constants, and the multi-GPU refusal."""
import math
import os
import re

import numpy as np
import pytest

import with_time_ref as W
from pinot_amd import _lib as L
from pinot_amd import parse_sql
from pinot_amd import query as Q
from pinot_amd.engine import (INT_MAX, INT_MIN, LONG_MAX, LONG_MIN, UnsupportedQuery, ValueTimePair, java_cast,
                              with_time_default)
from pinot_amd.filter_stats import projected_columns
from pinot_amd.reduce import final_value, merge_intermediate, merge_value

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ parser
@pytest.mark.parametrize("spelling", ["LASTWITHTIME", "lastwithtime", "LastWithTime", "lastWithTime", "LAST_WITH_TIME",
                                      "last_with_time", "Last_With_Time"])
def test_spellings_and_case(spelling):
    q = parse_sql("SELECT %s(intColumn, timestampColumn, 'int') FROM testTable" % spelling)
    a = q.aggregations[0]
    assert (a.function, a.column, a.time_column, a.data_type) == ("LASTWITHTIME", "intColumn", "timestampColumn", "INT")
    first = spelling.replace("Last", "First").replace("last", "first").replace("LAST", "FIRST")
    f = parse_sql("SELECT %s(intColumn, timestampColumn, 'Long') FROM testTable" % first).aggregations[0]
    assert (f.function, f.data_type) == ("FIRSTWITHTIME", "LONG")


def test_result_column_names_are_the_references():
    """LastWithTimeQueriesTest.java:239-244 (and the firstwithtime analogues): lower-case function, no spaces, the type
    literal upper-cased."""
    q = parse_sql("SELECT LASTWITHTIME(boolColumn, timestampColumn, 'boolean'), LASTWITHTIME(intColumn, timestampColumn, "
                  "'INT'), LASTWITHTIME(longColumn,timestampColumn,'long'), FIRSTWITHTIME(intColumn, timestampColumn, "
                  "'Int'), first_with_time(stringColumn, timestampColumn, 'STRING') FROM testTable")
    assert [a.result_name for a in q.aggregations] == [
        "lastwithtime(boolColumn,timestampColumn,'BOOLEAN')", "lastwithtime(intColumn,timestampColumn,'INT')",
        "lastwithtime(longColumn,timestampColumn,'LONG')", "firstwithtime(intColumn,timestampColumn,'INT')",
        "firstwithtime(stringColumn,timestampColumn,'STRING')"]
    assert q.columns() == {"boolColumn", "intColumn", "longColumn", "stringColumn", "timestampColumn"}
    assert "timestampColumn" in Q.query_columns(q)


def test_existing_positional_construction_keeps_working():
    a = Q.Aggregation("SUM", "m", 8, -1.0, 0, None)
    assert a.time_column is None and a.data_type == "" and a.function_name == "sum(m)"


@pytest.mark.parametrize("sql,message", [
    ("SELECT LASTWITHTIME(a, ts) FROM t", "LAST_WITH_TIME expects 3 arguments, got: 2. The function can be used as "
                                          "lastWithTime(dataColumn, timeColumn, 'dataType')"),
    ("SELECT FIRSTWITHTIME(a, ts, 'INT', 4) FROM t", "FIRST_WITH_TIME expects 3 arguments, got: 4. The function can be "
                                                     "used as firstWithTime(dataColumn, timeColumn, 'dataType')"),
    ("SELECT LASTWITHTIME(a, ts, dataType) FROM t", "LAST_WITH_TIME expects the 3rd argument to be literal, got: "
                                                    "IDENTIFIER. The function can be used as lastWithTime(dataColumn, "
                                                    "timeColumn, 'dataType')"),
    ("SELECT first_with_time(a, ts, upper(x)) FROM t", "FIRST_WITH_TIME expects the 3rd argument to be literal, got: "
                                                       "FUNCTION. The function can be used as firstWithTime(dataColumn, "
                                                       "timeColumn, 'dataType')"),
    ("SELECT LASTWITHTIME(a, ts, 'BYTES') FROM t", "Unsupported data type for LAST_WITH_TIME: BYTES"),
    ("SELECT FIRSTWITHTIME(a, ts, 'timestamp') FROM t", "Unsupported data type for FIRST_WITH_TIME: TIMESTAMP"),
    ("SELECT LASTWITHTIME(a, ts, 'number') FROM t", "No enum constant org.apache.pinot.spi.data.FieldSpec.DataType.NUMBER"),
])
def test_factory_errors(sql, message):
    with pytest.raises(ValueError) as e:
        parse_sql(sql)
    assert str(e.value) == message


def test_filter_clause_and_order_by_parse():
    q = parse_sql("SELECT g, LASTWITHTIME(v, ts, 'LONG') FILTER (WHERE x > 3) FROM t GROUP BY g "
                  "ORDER BY lastwithtime(v, ts, 'long') DESC LIMIT 3")
    assert q.aggregations[0].filter is not None and q.aggregations[0].result_name.endswith("FILTER(WHERE x > '3')")
    assert q.order_by[0].expr == q.aggregations[1] and not q.order_by[0].asc


def test_projected_columns_count_the_time_column_once():
    """Six value columns + the time column: 7 x docs (LastWithTimeQueriesTest.java:225); a group-by column that is also
    a value column adds nothing (:329)."""
    sel = ", ".join("LASTWITHTIME(%s, ts, '%s')" % (c, t) for c, t in
                    [("b", "BOOLEAN"), ("i", "INT"), ("l", "LONG"), ("f", "FLOAT"), ("d", "DOUBLE"), ("s", "STRING")])
    assert projected_columns(parse_sql("SELECT %s FROM t" % sel)) == 7
    assert projected_columns(parse_sql("SELECT %s FROM t GROUP BY i" % sel)) == 7


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("function", ["LASTWITHTIME", "FIRSTWITHTIME"])
def test_restatement_agrees_with_a_brute_force_sort(function):
    rng = np.random.default_rng(5)
    segments = []
    for n in (300, 1, 77, 0, 150):
        # 4 distinct times: ties inside and across segments are the rule
        segments.append((rng.integers(-2, 2, size=n), [int(k) for k in rng.integers(0, 9, size=n)], rng.random(n) < 0.7))
    assert W.table_winners(function, segments) == W.brute_force(function, segments)
    one = [(t, None, m) for t, _, m in segments]
    assert W.table_winners(function, one) == W.brute_force(function, one)
    # the extremes of the time domain beat nothing but each other
    ext = [(np.array([LONG_MIN, LONG_MAX, LONG_MIN, LONG_MAX]), None, [True] * 4)]
    assert W.table_winners("LASTWITHTIME", ext) == {(): (0, 3, LONG_MAX)}
    assert W.table_winners("FIRSTWITHTIME", ext) == {(): (0, 2, LONG_MIN)}


def test_restatement_group_limit_admits_first_seen_keys():
    keys = [3, 3, 1, 2, 1, 2, 3]
    seg = (np.arange(7), keys, [True] * 7)
    assert W.table_winners("LASTWITHTIME", [seg], limit=2) == {3: (0, 6, 6), 1: (0, 4, 4)}


# ------------------------------------------------------------------ broker
def test_merge_value_first_argument_wins_equal_times():
    a, b = ValueTimePair(1, 10), ValueTimePair(2, 10)
    assert merge_value("LASTWITHTIME", a, b) is a and merge_value("LASTWITHTIME", b, a) is b
    assert merge_value("FIRSTWITHTIME", a, b) is a and merge_value("FIRSTWITHTIME", b, a) is b
    late = ValueTimePair(3, 11)
    assert merge_value("LASTWITHTIME", a, late) is late and merge_value("LASTWITHTIME", late, a) is late
    assert merge_value("FIRSTWITHTIME", a, late) is a and merge_value("FIRSTWITHTIME", late, a) is a


def test_a_doc_at_the_time_domains_end_beats_the_default_in_the_merge():
    """The default pair as the first argument: LAST keeps a when a.time >= b.time, so a doc at Long.MIN_VALUE loses the
    broker merge to a default on its left exactly as in the reference (merge, :223); on the server the doc wins
    (test_gpu_with_time)."""
    d = with_time_default("LASTWITHTIME", "LONG")
    doc = ValueTimePair(7, LONG_MIN)
    assert merge_value("LASTWITHTIME", doc, d) is doc and merge_value("LASTWITHTIME", d, doc) is d


def test_default_pairs_and_final_values():
    for fn, t in (("LASTWITHTIME", LONG_MIN), ("FIRSTWITHTIME", LONG_MAX)):
        assert with_time_default(fn, "INT") == ValueTimePair(INT_MIN, t)
        assert with_time_default(fn, "BOOLEAN") == ValueTimePair(INT_MIN, t)
        assert with_time_default(fn, "LONG") == ValueTimePair(LONG_MIN, t)
        assert with_time_default(fn, "STRING") == ValueTimePair("", t)
        for dt in ("FLOAT", "DOUBLE"):
            p = with_time_default(fn, dt)
            assert math.isnan(p.value) and p.time == t and p == with_time_default(fn, dt)
        q = parse_sql("SELECT %s(a, ts, 'INT'), %s(a, ts, 'BOOLEAN'), %s(s, ts, 'STRING') FROM t" % (fn, fn, fn))
        row = [with_time_default(fn, a.data_type) for a in q.aggregations]
        assert [final_value(a, v) for a, v in zip(q.aggregations, row)] == [INT_MIN, True, ""]
    assert final_value("LASTWITHTIME", ValueTimePair(5.5, 1)) == 5.5
    b = parse_sql("SELECT LASTWITHTIME(a, ts, 'BOOLEAN') FROM t").aggregations[0]
    assert final_value(b, ValueTimePair(0, 1)) is False and final_value(b, ValueTimePair(-3, 1)) is True


def test_merge_intermediate_merges_pairs():
    from pinot_amd.engine import IntermediateResult
    q = parse_sql("SELECT g, LASTWITHTIME(a, ts, 'INT'), FIRSTWITHTIME(a, ts, 'INT') FROM t GROUP BY g")
    r1 = IntermediateResult(q.aggregations, q.group_by, {(1,): [ValueTimePair(1, 5), ValueTimePair(1, 5)]})
    r2 = IntermediateResult(q.aggregations, q.group_by, {(1,): [ValueTimePair(2, 9), ValueTimePair(2, 9)],
                                                         (2,): [ValueTimePair(3, 0), ValueTimePair(3, 0)]})
    m = merge_intermediate([r1, r2])
    assert m.groups == {(1,): [ValueTimePair(2, 9), ValueTimePair(1, 5)], (2,): [ValueTimePair(3, 0), ValueTimePair(3, 0)]}


# ------------------------------------------------------------------ the declared type's getter
def test_java_casts():
    assert java_cast(np.int64(0x1_2345_6789), "LONG", "INT") == 0x2345_6789           # long -> int: the low 32 bits
    assert java_cast(np.int64(0x1_8000_0001), "LONG", "INT") == INT_MIN + 1
    assert java_cast(np.int64(-1), "LONG", "INT") == -1
    assert java_cast(np.int32(-7), "INT", "LONG") == -7
    assert java_cast(1e30, "DOUBLE", "LONG") == LONG_MAX and java_cast(-1e30, "DOUBLE", "LONG") == LONG_MIN
    assert java_cast(float(2 ** 63), "DOUBLE", "LONG") == LONG_MAX
    assert java_cast(1e30, "DOUBLE", "INT") == INT_MAX and java_cast(np.float32(-3e9), "FLOAT", "INT") == INT_MIN
    assert java_cast(float("nan"), "DOUBLE", "LONG") == 0 and java_cast(float("nan"), "FLOAT", "INT") == 0
    assert java_cast(-2.9, "DOUBLE", "INT") == -2 and java_cast(2.9, "DOUBLE", "LONG") == 2   # toward zero
    assert java_cast(np.int32(0), "INT", "BOOLEAN") == 0 and java_cast(np.int32(5), "INT", "BOOLEAN") == 5
    assert java_cast(np.int64(1 << 40), "LONG", "FLOAT") == float(np.float32(1 << 40))
    assert java_cast(0.1, "DOUBLE", "FLOAT") == float(np.float32(0.1)) and java_cast(1e300, "DOUBLE", "FLOAT") == math.inf
    assert java_cast(np.float32(0.1), "FLOAT", "DOUBLE") == float(np.float32(0.1))
    assert java_cast(np.int64((1 << 53) + 1), "LONG", "DOUBLE") == float(1 << 53)
    assert java_cast("abc", "STRING", "STRING") == "abc"
    with pytest.raises(UnsupportedQuery):
        java_cast(3, "INT", "STRING")
    with pytest.raises(UnsupportedQuery):
        java_cast("abc", "STRING", "LONG")


# ------------------------------------------------------------------ C-ABI declarations, multi-GPU
def test_abi_declarations():
    header = open(os.path.join(ROOT, "include", "pinot_amd.h")).read()
    assert L.PA_AGG_LAST_ROW_BY_TIME == 8 and L.PA_AGG_FIRST_ROW_BY_TIME == 9
    assert L.PA_ACC_TIME_ROW_U64 == 13 and L.PA_ACC_TIME_MAX_I64 == 14
    for name, value in (("PA_AGG_LAST_ROW_BY_TIME", 8), ("PA_AGG_FIRST_ROW_BY_TIME", 9), ("PA_ACC_TIME_ROW_U64", 13),
                        ("PA_ACC_TIME_MAX_I64", 14)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert re.search(r"#define PA_ABI_VERSION %d\b" % L.ABI_VERSION, header)
    assert re.search(r"int pa_query_fetch_time_rows\(pa_query\* q, void\* stream, int32_t agg, int64_t num_groups, "
                     r"int32_t num_columns,\s+const int32_t\* columns, int32_t\* out_segments, int32_t\* out_docs, "
                     r"int64_t\* const\* out_cells\);", header)
    assert re.search(r"int32_t pa_query_time_row_form\(const pa_query\* q, int32_t agg\);", header)
    assert {"pa_query_fetch_time_rows", "pa_query_time_row_form"} <= set(L.EXPORTED)
    tuning = open(os.path.join(ROOT, "pinot_amd", "csrc", "pa_tuning.h")).read()
    assert re.search(r"X\(time_rows_wide, -1, 0, 1, 0\)", tuning)


def test_distributed_query_is_refused_before_any_collective():
    """The new sections are not element-wise reducible: UnsupportedQuery with the reason, not a KeyError from the
    reduce-op tables, and nothing is sent (no process group exists here: a collective would raise something else)."""
    from pinot_amd import parallel
    assert parallel.SECTION_OP[L.PA_ACC_TIME_ROW_U64] is None and parallel.SECTION_OP[L.PA_ACC_TIME_MAX_I64] is None
    assert L.PA_ACC_TIME_ROW_U64 in parallel.SECTION_DTYPE and L.PA_ACC_TIME_MAX_I64 in parallel.SECTION_DTYPE
    q = parse_sql("SELECT g, LASTWITHTIME(v, ts, 'LONG') FROM t GROUP BY g")
    with pytest.raises(UnsupportedQuery, match="rank"):
        parallel.table_layout(q, [])

    class Executor:
        query, handle, hashed = q, 1, False
    with pytest.raises(UnsupportedQuery, match="not element-wise reducible"):
        parallel.DistributedAccumulators(Executor(), "cpu")
