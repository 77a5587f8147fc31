"""Transform expressions on the host: the parser (spellings, precedence, unary minus against subtraction, canonical
names, existing queries unchanged), type inference, the lowering order, transform.evaluate against hand-computed values,
every refusal the host decides, the reduce-level merge of expression keys, and the reference's golden results
(tests/golden/transform_queries.json, transcribed from TransformQueriesTest.java) through the numpy restatement.
tests/test_gpu_transform.py runs CASES and the golden file on the GPU."""
import json
import math
import os

import numpy as np
import pytest

import transform_ref as R
from pinot_amd import parse_sql
from pinot_amd import query as Q
from pinot_amd import transform as T
from pinot_amd.engine import IntermediateResult, UnsupportedQuery
from pinot_amd.reduce import final_result_table, merge_intermediate
from pinot_amd.segment import create_segment

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "transform_queries.json")))

SCHEMA = {"g": "INT", "h": "INT", "f": "INT", "di": "INT", "dl": "LONG", "df": "FLOAT", "dd": "DOUBLE", "ri": "INT",
          "rl": "LONG", "rd": "DOUBLE", "ts": "LONG", "s": "STRING"}
RAW = ["ri", "rl", "rd", "ts"]


def make_segment(name, n, seed, shift=0):
    """n docs. Every value is an integer or a multiple of 1/4 of small magnitude, so sums of + - * results are exact in
    any order; dl holds values past int32, ts millisecond timestamps either side of the epoch."""
    rng = np.random.default_rng(seed)
    data = {
        "g": rng.integers(0, 5, n) + shift, "h": rng.integers(0, 3, n), "f": rng.integers(0, 100, n),
        "di": rng.integers(-20, 20, n) + shift, "dl": (rng.integers(-8, 8, n).astype(np.int64) << 33) + shift,
        "df": (rng.integers(1, 16, n) * 0.5).astype(np.float32), "dd": rng.integers(-40, 40, n) * 0.25 + shift,
        "ri": rng.integers(-50, 50, n), "rl": rng.integers(-2**40, 2**40, n), "rd": rng.integers(-64, 64, n) * 0.25,
        "ts": rng.integers(-3 * 86400000, 5 * 86400000, n), "s": np.array(["x%d" % (i % 3) for i in range(n)], dtype=object),
    }
    return create_segment(name, data, SCHEMA, no_dictionary_columns=RAW)


def make_table(n):
    """One segment of n docs with its own dictionaries next to two that share theirs (the same data)."""
    return [make_segment("own_%d" % n, n, 100 + n, shift=3), make_segment("shared_a", 300, 7), make_segment("shared_b", 300, 7)]


# one query per shape the scan treats differently; (sql, exact DOUBLE sums)
CASES = {
    "aggregation_only": ("SELECT SUM(ADD(di, dl)), MIN(SUB(dd, ri)), MAX(MULT(df, 2, di)), AVG(rd * 4 + ri), "
                         "MINMAXRANGE(ABS(SUB(ri, di))), COUNT(*), SUM(di), MAX(rl) FROM t", True),
    "nested_literals": ("SELECT SUM(ADD(1, MULT(SUB(dl, 3), CEIL(DIV(ri, 4))), 2)), MAX(FLOOR(dd / 2) - 1), "
                        "MIN(2 - MOD(ri, 7)) FROM t WHERE f < 50", True),
    "group_by_columns": ("SELECT g, h, SUM(ADD(di, ri)), MAX(FLOOR(dd)), AVG(df * rd), SUM(dl), COUNT(*) FROM t "
                         "GROUP BY g, h LIMIT 1000", True),
    "group_by_long_expr": ("SELECT timeConvert(ts, 'MILLISECONDS', 'DAYS'), COUNT(*), SUM(rl), "
                           "SUM(timeConvert(ts, 'MILLISECONDS', 'SECONDS')), MAX(timeConvert(ts, 'SECONDS', 'MICROSECONDS')) "
                           "FROM t GROUP BY timeConvert(ts, 'MILLISECONDS', 'DAYS') LIMIT 1000", True),
    "group_by_double_expr": ("SELECT COUNT(*), SUM(di), MIN(ri + dd) FROM t WHERE f >= 10 "
                             "GROUP BY ADD(MOD(ri, 7), 0.5) LIMIT 1000", True),  # (-0.0 keys: test_gpu_transform's own case)
    "group_by_column_and_expr": ("SELECT g, SUM(dd), COUNT(*), MAX(SUB(di, ri)) FROM t GROUP BY g, ADD(di, ri) LIMIT 100000",
                                 True),
    "sparse_filter": ("SELECT h, SUM(MULT(di, ri)), SUM(ADD(di, 1)), COUNT(*) FROM t WHERE f = 3 GROUP BY h LIMIT 1000", True),
    "inexact_sums": ("SELECT g, SUM(DIV(dd, df)), AVG(SUB(DIV(rd, 3), DIV(dd, 7))), COUNT(*) FROM t GROUP BY g LIMIT 1000",
                     False),
}

EXISTING_SPELLINGS = [
    "SELECT COUNT(*) FROM t",
    "SELECT SUM(x), MIN(y), AVG(z) FROM t WHERE a = -1 AND b BETWEEN -5 AND -2 GROUP BY g, h ORDER BY SUM(x) DESC LIMIT 5",
    "SELECT g, DISTINCTCOUNTHLL(x, 12), PERCENTILE(y, 95), PERCENTILE50(y) FROM t WHERE c IN (1, -2, 3) GROUP BY g ORDER BY g",
    "SELECT SUM(x) FILTER (WHERE a > -3) AS s, COUNT(*) FROM t GROUP BY g ORDER BY s",
    "SELECT a, b FROM t WHERE c <> -1.5e3 ORDER BY a DESC, b LIMIT 3, 10",
    "SELECT DISTINCT a, b FROM t ORDER BY b LIMIT 7",
]


def _agg(sql, i=0):
    return parse_sql(sql).aggregations[i]


def _expr(text):
    return _agg("SELECT SUM(%s) FROM t" % text).column


# ------------------------------------------------------------------ parser
def test_parses_what_the_parent_refused():
    assert _agg("SELECT SUM(ADD(a,b)) FROM t").column == Q.Expr("add", (("id", "a"), ("id", "b")))


@pytest.mark.parametrize("text,canonical", [
    ("ADD(a, b)", "add(a,b)"), ("plus(a,b)", "plus(a,b)"), ("a + b", "plus(a,b)"),
    ("MULT(a,b,c)", "mult(a,b,c)"), ("times(a,b)", "times(a,b)"), ("a * b", "times(a,b)"),
    ("SUB(a,b)", "sub(a,b)"), ("minus(a,b)", "minus(a,b)"), ("a - b", "minus(a,b)"),
    ("DIV(a,b)", "div(a,b)"), ("divide(a,b)", "divide(a,b)"), ("a / b", "divide(a,b)"),
    ("MOD(a,b)", "mod(a,b)"), ("a % b", "mod(a,b)"),
    ("ABS(a)", "abs(a)"), ("CEIL(a)", "ceil(a)"), ("ceiling(a)", "ceiling(a)"), ("Floor(a)", "floor(a)"),
    ("timeConvert(ts, 'MILLISECONDS', 'DAYS')", "timeconvert(ts,'MILLISECONDS','DAYS')"),
    ("TIME_CONVERT(ts, 'SECONDS', 'HOURS')", "timeconvert(ts,'SECONDS','HOURS')"),
    ("ADD(a, 1.5)", "add(a,'1.5')"),
])
def test_spellings(text, canonical):
    e = _expr(text)
    assert str(e) == canonical
    T.validate(e)


def test_precedence_and_associativity():
    assert str(_expr("a + b * c")) == "plus(a,times(b,c))"
    assert str(_expr("a * b + c")) == "plus(times(a,b),c)"
    assert str(_expr("a + b + c")) == "plus(plus(a,b),c)"   # Calcite builds binary calls
    assert str(_expr("a - b - c")) == "minus(minus(a,b),c)"
    assert str(_expr("a / b % c * d")) == "times(mod(divide(a,b),c),d)"
    assert str(_expr("(a + b) * (c - d)")) == "times(plus(a,b),minus(c,d))"
    assert str(_expr("a - ABS(b) * 2")) == "minus(a,times(abs(b),'2'))"


def test_minus_is_subtraction_after_an_operand():
    assert str(_expr("a -1")) == "minus(a,'1')"
    assert str(_expr("a-1")) == "minus(a,'1')"
    assert str(_expr("(a) -1")) == "minus(a,'1')"
    assert str(_expr("ABS(a) - 2.5")) == "minus(abs(a),'2.5')"
    assert str(_expr("ADD(a, -1)")) == "add(a,'-1')"
    assert str(_expr("a * -2")) == "times(a,'-2')"
    q = parse_sql("SELECT COUNT(*) FROM t WHERE a = -1 AND b BETWEEN -5 AND -2 AND c IN (-1, -2)")
    assert q.filter == Q.And((Q.EqPredicate("a", "-1"), Q.RangePredicate("b", "-5", True, "-2", True),
                              Q.InPredicate("c", ("-1", "-2"))))


def test_canonical_names_of_the_reference():
    # ForwardIndexDisabledSingleValueQueriesTest.java:1604 and :1639
    assert _agg("SELECT MAX(ADD(column1, column9)) FROM testTable").result_name == "max(add(column1,column9))"
    q = parse_sql("SELECT column1, MAX(ADD(column1, column9)) FROM testTable GROUP BY column1")
    assert [q.select_columns[0], q.aggregations[0].result_name] == ["column1", "max(add(column1,column9))"]
    assert _agg("SELECT sum(a + b) FROM t").result_name == "sum(plus(a,b))"
    assert _agg("SELECT AVG(SUB(INT_COL1, INT_COL2)) FROM t").result_name == "avg(sub(INT_COL1,INT_COL2))"


def test_existing_queries_parse_to_the_same_objects():
    for sql in EXISTING_SPELLINGS:
        q = parse_sql(sql)
        assert all(isinstance(g, str) for g in q.group_by), sql
        assert all(a.column is None or isinstance(a.column, str) for a in q.aggregations), sql
        assert all(isinstance(c, str) for c in q.select_columns), sql
        assert all(isinstance(o.expr, (str, Q.Aggregation)) for o in q.order_by), sql
    q = parse_sql(EXISTING_SPELLINGS[1])
    assert q.aggregations == [Q.Aggregation("SUM", "x"), Q.Aggregation("MIN", "y"), Q.Aggregation("AVG", "z")]
    assert q.group_by == ["g", "h"] and q.order_by == [Q.OrderBy(Q.Aggregation("SUM", "x"), False)] and q.limit == 5
    assert q.filter == Q.And((Q.EqPredicate("a", "-1"), Q.RangePredicate("b", "-5", True, "-2", True)))
    q = parse_sql(EXISTING_SPELLINGS[4])
    assert q.select_columns == ["a", "b"] and (q.offset, q.limit) == (3, 10)
    assert q.filter == Q.NotEqPredicate("c", "-1.5e3")


def test_group_by_select_list_order_by_and_columns():
    q = parse_sql("SELECT timeConvert(ts,'MILLISECONDS','DAYS'), g, SUM(a * b) FROM t WHERE f = 1 "
                  "GROUP BY timeConvert(ts,'MILLISECONDS','DAYS'), g ORDER BY timeConvert(ts,'MILLISECONDS','DAYS') DESC, "
                  "SUM(a * b)")
    e = q.group_by[0]
    assert isinstance(e, Q.Expr) and q.group_by[1] == "g" and q.select_columns == [e, "g"]
    assert q.order_by == [Q.OrderBy(e, False), Q.OrderBy(q.aggregations[0], True)]
    assert q.columns() == {"ts", "g", "a", "b", "f"}
    assert Q.query_columns(q) == ["f", "ts", "g", "a", "b"]


# ------------------------------------------------------------------ types and lowering
def test_type_inference():
    assert T.infer_type(_expr("ADD(a, b)")) == T.DOUBLE
    assert T.infer_type(_expr("timeConvert(a, 'DAYS', 'HOURS')")) == T.LONG
    assert T.infer_type(_expr("ADD(timeConvert(a, 'DAYS', 'HOURS'), 1)")) == T.DOUBLE
    assert T.infer_type(_expr("FLOOR(a)")) == T.DOUBLE
    assert T.evaluate(_expr("timeConvert(a, 'DAYS', 'HOURS')"), {"a": np.array([2], np.int32)}).dtype == np.int64
    assert T.evaluate(_expr("ABS(a)"), {"a": np.array([2], np.int32)}).dtype == np.float64


def test_lowering_order():
    assert T.lower(_expr("ADD(1, a, 2, b)")).infix() == "((3.0 + a) + b)"   # literal terms folded first
    assert T.lower(_expr("ADD(a, b)")).infix() == "((0.0 + a) + b)"
    assert T.lower(_expr("MULT(2, a, 4, b, c)")).infix() == "(((8.0 * a) * b) * c)"
    assert T.lower(_expr("a + b + c")).infix() == "((0.0 + ((0.0 + a) + b)) + c)"
    assert T.lower(_expr("SUB(3, a)")).infix() == "(3.0 - a)"
    assert T.lower(_expr("DIV(MOD(a, 2), ABS(b))")).infix() == "((a % 2.0) / abs(b))"
    assert T.lower(_expr("timeConvert(a, 'MILLISECONDS', 'DAYS')")).infix() == "tdiv(long(a), 86400000)"
    assert T.lower(_expr("timeConvert(a, 'HOURS', 'SECONDS')")).infix() == "tmul(long(a), 3600)"
    assert T.lower(_expr("timeConvert(a, 'HOURS', 'HOURS')")).infix() == "long(a)"
    assert T.lower(_expr("timeConvert(ADD(a, 1), 'HOURS', 'DAYS')")).infix() == "tdiv(d2l((1.0 + a)), 24)"
    assert T.lower(_expr("SUB(timeConvert(a, 'DAYS', 'HOURS'), b)")).infix() == "(l2d(tmul(long(a), 24)) - b)"
    p = T.lower(_expr("ADD(a, MULT(a, b))"))
    assert p.columns == ["a", "b"] and len(p.ops) == 7   # (a is one operand column, loaded by each use)


def test_negative_zero_operand_becomes_positive_zero():
    z = T.evaluate(_expr("ADD(a, b)"), {"a": np.array([-0.0]), "b": np.array([-0.0])})
    assert z[0] == 0.0 and not math.copysign(1.0, z[0]) < 0   # (0.0 + -0.0) + -0.0 = +0.0
    z = T.evaluate(_expr("MULT(a, b)"), {"a": np.array([-0.0]), "b": np.array([3.0])})
    assert math.copysign(1.0, z[0]) < 0                        # (1.0 * -0.0) * 3.0 = -0.0
    z = T.evaluate(_expr("SUB(a, b)"), {"a": np.array([-0.0]), "b": np.array([0.0])})
    assert math.copysign(1.0, z[0]) < 0


# ------------------------------------------------------------------ evaluate against hand-computed values
def test_evaluate_division_and_modulo():
    v = T.evaluate(_expr("DIV(a, b)"), {"a": np.array([1, -1, 0, 7]), "b": np.array([0, 0, 0, 2])})
    assert v[0] == math.inf and v[1] == -math.inf and math.isnan(v[2]) and v[3] == 3.5
    v = T.evaluate(_expr("MOD(a, b)"), {"a": np.array([7, -7, 7, -7, 5.5, 1]), "b": np.array([3, 3, -3, -3, 2, 0])})
    assert v[:5].tolist() == [1.0, -1.0, 1.0, -1.0, 1.5] and math.isnan(v[5])   # Java %: the dividend's sign
    v = T.evaluate(_expr("ABS(a) + CEIL(b) * FLOOR(b)"), {"a": np.array([-2.5, 2.5]), "b": np.array([-1.5, 1.5])})
    assert v.tolist() == [2.5 + (-1.0 * -2.0), 2.5 + 2.0 * 1.0]


def test_evaluate_long_past_2_53_loses_precision_as_the_reference():
    big = 2**53 + 1
    v = T.evaluate(_expr("ADD(a, b)"), {"a": np.array([big], np.int64), "b": np.array([0], np.int64)})
    assert v[0] == float(2**53)          # (double)(2^53 + 1) = 2^53
    v = T.evaluate(_expr("SUB(a, b)"), {"a": np.array([big], np.int64), "b": np.array([2**53], np.int64)})
    assert v[0] == 0.0
    v = T.evaluate(_expr("ADD(a, 0)"), {"a": np.array([1.5], np.float32)})
    assert v[0] == 1.5                   # FLOAT widens


def test_evaluate_timeconvert():
    day = 86400000
    v = T.evaluate(_expr("timeConvert(a, 'MILLISECONDS', 'DAYS')"),
                   {"a": np.array([-1, -day, -day - 1, day - 1, day, 0], np.int64)})
    assert v.tolist() == [0, -1, -1, 0, 1, 0]           # truncation toward zero
    v = T.evaluate(_expr("timeConvert(a, 'DAYS', 'NANOSECONDS')"),
                   {"a": np.array([1, -1, 106751, 106752, -106751, -106752, 2**62, -2**62], np.int64)})
    ns = 86400 * 10**9
    assert v.tolist() == [ns, -ns, 106751 * ns, 2**63 - 1, -106751 * ns, -2**63, 2**63 - 1, -2**63]  # saturating
    v = T.evaluate(_expr("timeConvert(a, 'SECONDS', 'SECONDS')"), {"a": np.array([-5, 7], np.int32)})
    assert v.tolist() == [-5, 7]
    # a DOUBLE argument goes through Java's (long) cast
    v = T.evaluate(_expr("timeConvert(a, 'SECONDS', 'SECONDS')"),
                   {"a": np.array([math.nan, math.inf, -math.inf, 1e30, -1e30, -2.9, 2.9])})
    assert v.tolist() == [0, 2**63 - 1, -2**63, 2**63 - 1, -2**63, -2, 2]
    v = T.evaluate(_expr("timeConvert(DIV(a, 0), 'SECONDS', 'MILLISECONDS')"), {"a": np.array([1, -1, 0])})
    assert v.tolist() == [2**63 - 1, -2**63, 0]


# ------------------------------------------------------------------ refusals
SCHEMA_SV = {n: (t, True) for n, t in SCHEMA.items()}
SCHEMA_SV["mv"] = ("INT", False)
SCHEMA_SV["b"] = ("BYTES", True)


@pytest.mark.parametrize("sql,match", [
    ("SELECT COUNT(*) FROM t GROUP BY DATETRUNC('week', ts, 'SECONDS')", "transform function datetrunc"),
    ("SELECT COUNT(*) FROM t GROUP BY DATETIMECONVERT(ts, '1:MILLISECONDS:EPOCH', '1:DAYS:EPOCH', '1:DAYS')",
     "transform function datetimeconvert"),
    ("SELECT SUM(CASE WHEN di > 1 THEN ri ELSE 0 END) FROM t", "transform function case"),
    ("SELECT SUM(CAST(di AS LONG)) FROM t", "transform function cast"),
    ("SELECT SUM(EXP(di)) FROM t", "transform function exp"),
    ("SELECT SUM(LN(di)) FROM t", "transform function ln"),
    ("SELECT SUM(SQRT(di)) FROM t", "transform function sqrt"),
    ("SELECT SUM(POWER(di, 2)) FROM t", "transform function power"),
    ("SELECT SUM(FOO(di)) FROM t", "transform function foo"),
    ("SELECT COUNT(*) FROM t GROUP BY timeConvert(ts, 'MILLISECONDS', 'WEEKS')", "custom time unit WEEKS"),
    ("SELECT COUNT(*) FROM t GROUP BY timeConvert(ts, 'MILLISECONDS', 'MONTHS')", "custom time unit MONTHS"),
    ("SELECT COUNT(*) FROM t GROUP BY timeConvert(ts, 'MILLISECONDS', 'YEARS')", "custom time unit YEARS"),
    ("SELECT SUM(SUB(di, s)) FROM t", "STRING column s"),
    ("SELECT SUM(ADD(di, b)) FROM t", "BYTES column b"),
    ("SELECT SUM(ADD(di, mv)) FROM t", "multi-value column mv"),
    ("SELECT SUM(ADD(di, nope)) FROM t", "unknown column nope"),
    ("SELECT SUM(ADD(1, 2)) FROM t", "only of literals"),
    ("SELECT SUM(ADD(di, MULT(2, 3))) FROM t", "only of literals"),
    ("SELECT PERCENTILE(ADD(di, ri), 50) FROM t", "PERCENTILE over the transform expression"),
    ("SELECT DISTINCTCOUNT(ADD(di, ri)) FROM t", "DISTINCTCOUNT over the transform expression"),
    ("SELECT DISTINCTCOUNTHLL(ADD(di, ri)) FROM t", "DISTINCTCOUNTHLL over the transform expression"),
    ("SELECT SUM(ADD(di, ri)) FILTER (WHERE f = 1) FROM t", "aggregation filters"),
    ("SELECT SUM(ADD(di, ri)), COUNT(*) FILTER (WHERE f = 1) FROM t", "aggregation filters"),
    ("SELECT SUM(ADD(di, ri)) FROM t OPTION(enableNullHandling=true)", "null handling"),
    ("SELECT ADD(di, ri) FROM t", "in a selection"),
    ("SELECT di FROM t ORDER BY ADD(di, ri)", "in a selection"),
    ("SELECT " + ", ".join("SUM(ADD(di, %d))" % i for i in range(9)) + " FROM t", "more than 8 transform expressions"),
    ("SELECT SUM(ADD(" + ", ".join(["di"] * 9) + ")) FROM t", "more than 16 operations"),
    ("SELECT SUM(ADD(g, h, f, di, dl, df, dd, ri, rl)) FROM t", "more than 8 distinct columns"),
    # nine operands alive at once: every SUB holds its left operand while the right one is evaluated
    ("SELECT SUM(" + "SUB(di, " * 8 + "di" + ")" * 8 + ") FROM t", "more than 8 value registers"),
])
def test_refused(sql, match):
    with pytest.raises(UnsupportedQuery, match=match):
        T.check_query(parse_sql(sql), SCHEMA_SV)


@pytest.mark.parametrize("sql", ["SELECT DISTINCT ADD(di, ri) FROM t", "SELECT COUNT(*) FROM t WHERE di + ri > 3",
                                 "SELECT COUNT(*) FILTER (WHERE di + ri > 3) FROM t", "SELECT SUM(-di) FROM t"])
def test_refused_by_the_parser_as_before(sql):
    with pytest.raises(ValueError):
        parse_sql(sql)


@pytest.mark.parametrize("text,message", [
    ("ADD(a)", "At least 2 arguments are required for ADD transform function"),
    ("SUB(a, b, c)", "Exactly 2 arguments are required for SUB transform function"),
    ("DIV(a)", "Exactly 2 arguments are required for DIV transform function"),
    ("MOD(a, b, c)", "Exactly 2 arguments are required for MOD transform function"),
    ("ABS(a, b)", "Exactly 1 argument is required for ABS transform function"),
    ("timeConvert(a, 'DAYS')", "Exactly 3 arguments are required for TIME_CONVERT transform function"),
    ("timeConvert(5, 'DAYS', 'HOURS')", "The first argument of TIME_CONVERT transform function must be"),
    ("timeConvert(a, 'FORTNIGHTS', 'HOURS')", "No enum constant java.util.concurrent.TimeUnit.FORTNIGHTS"),
    ("timeConvert(a, 'WEEKS', 'HOURS')", "No enum constant java.util.concurrent.TimeUnit.WEEKS"),
])
def test_argument_errors(text, message):
    with pytest.raises(ValueError, match=message):
        T.validate(_expr(text))


def test_limits_accepted():
    exprs, programs, columns = T.check_query(parse_sql(
        "SELECT " + ", ".join("SUM(ADD(di, %d))" % i for i in range(8)) + " FROM t"), SCHEMA_SV)
    assert len(exprs) == 8 and columns == ["di"]
    _, programs, _ = T.check_query(parse_sql("SELECT SUM(ADD(" + ", ".join(["di"] * 8) + ")) FROM t"), SCHEMA_SV)
    assert len(programs[0].ops) == 16
    _, _, columns = T.check_query(parse_sql("SELECT SUM(ADD(g, h, f, di, dl, df, dd, ri)) FROM t"), SCHEMA_SV)
    assert len(columns) == 8


def test_eight_registers_accepted():
    _, programs, _ = T.check_query(parse_sql("SELECT SUM(" + "SUB(di, " * 7 + "di" + ")" * 7 + ") FROM t"), SCHEMA_SV)
    assert len({op[1] for op in programs[0].ops}) == 8 and len(programs[0].ops) == 15


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("n", [65, 5000])
def test_exact_flags_hold(name, n):
    """A case marked exact sums DOUBLE values whose partial sums are all doubles (transform_ref.sums_are_exact); the one
    marked inexact does not (its DIV results are not dyadic), so it is compared within the relative bound."""
    sql, exact = CASES[name]
    assert R.double_sums_exact(parse_sql(sql), make_table(n)) == exact


# ------------------------------------------------------------------ reduce
def test_merge_of_expression_keys():
    q = parse_sql("SELECT DIV(a, b), COUNT(*), SUM(a) FROM t GROUP BY DIV(a, b)")
    nan = float("nan")

    def part(rows):
        r = IntermediateResult(list(q.aggregations), list(q.group_by))
        r.groups = {(T.DoubleKey(k),): [c, s] for k, c, s in rows}
        return r
    a = part([(nan, 2, 1.0), (0.0, 1, 2.0), (-0.0, 4, 3.0), (math.inf, 1, 1.0), (2.5, 1, 5.0)])
    b = part([(-nan, 3, 4.0), (-0.0, 1, 1.0), (2.5, 2, 1.0), (-math.inf, 7, 0.0)])
    m = merge_intermediate([a, b])
    got = {R.key_bits(k): v for k, v in m.groups.items()}
    assert len(got) == len(m.groups) == 6
    assert got[R.key_bits((nan,))] == [5, 5.0]            # every NaN one group
    assert got[R.key_bits((0.0,))] == [1, 2.0]            # -0.0 and 0.0 two groups
    assert got[R.key_bits((-0.0,))] == [5, 4.0]
    assert got[R.key_bits((2.5,))] == [3, 6.0]
    assert got[R.key_bits((math.inf,))] == [1, 1.0] and got[R.key_bits((-math.inf,))] == [7, 0.0]
    assert all(isinstance(k[0], float) for k in m.groups)
    # LONG keys are ints; the result table names the key column by the canonical text
    ql = parse_sql("SELECT timeConvert(ts,'MILLISECONDS','DAYS'), COUNT(*) FROM t GROUP BY timeConvert(ts,'MILLISECONDS','DAYS') "
                   "ORDER BY timeConvert(ts,'MILLISECONDS','DAYS') DESC LIMIT 2")
    x, y = (IntermediateResult(list(ql.aggregations), list(ql.group_by)) for _ in range(2))
    x.groups = {(2**63 - 1,): [1], (-2**63,): [2], (5,): [3]}
    y.groups = {(2**63 - 1,): [4], (6,): [1]}
    m = merge_intermediate([x, y])
    assert m.groups == {(2**63 - 1,): [5], (-2**63,): [2], (5,): [3], (6,): [1]}
    assert final_result_table(m, ql) == [[2**63 - 1, 5], [6, 1]]
    assert str(ql.group_by[0]) == "timeconvert(ts,'MILLISECONDS','DAYS')"


# ------------------------------------------------------------------ the reference's golden results
def golden_segment(copy=0):
    rows = GOLDEN["rows"]
    data = {c: np.array([r[c] for r in rows], dtype=object if t == "STRING" else None) for c, t in GOLDEN["schema"].items()}
    return create_segment("testSegment%d" % copy, data, GOLDEN["schema"])


def test_golden_file_shape():
    assert len(GOLDEN["rows"]) == 10 and len(GOLDEN["inner_segment"]) == 7 and len(GOLDEN["inter_segment"]) == 7
    assert len(GOLDEN["failing"]) == 2 and len(GOLDEN["datetrunc_refused"]) == 3


@pytest.mark.parametrize("case", GOLDEN["inner_segment"], ids=lambda c: c["source"].rsplit(":", 1)[1])
def test_golden_inner_segment(case):
    seg = golden_segment()
    a = parse_sql(case["query"]).aggregations[0]
    v = R.expr_values(a.column, seg)
    assert (float(np.sum(v)), len(v)) == (case["sum"], case["count"])


@pytest.mark.parametrize("case", GOLDEN["inter_segment"], ids=lambda c: c["source"].rsplit(":", 1)[1])
def test_golden_inter_segment(case):
    """getBrokerResponse runs the two servers over [segment, segment]: four copies of the segment."""
    q = parse_sql(case["query"])
    ref, _ = R.reference(q, [golden_segment(i) for i in range(4)])
    assert ref.row[0].count == 40 and ref.row[0].sum / ref.row[0].count == case["avg"]


def test_golden_failing_and_datetrunc():
    schema = {n: (t, True) for n, t in GOLDEN["schema"].items()}
    for case in GOLDEN["failing"]:
        with pytest.raises(UnsupportedQuery, match="STRING column STRING_COL"):
            T.check_query(parse_sql(case["query"]), schema)
    for case in GOLDEN["datetrunc_refused"]:
        with pytest.raises(UnsupportedQuery, match="transform function datetrunc"):
            T.check_query(parse_sql(case["query"]), schema)


# ------------------------------------------------------------------ the reference method itself
@pytest.mark.parametrize("name", sorted(CASES))
def test_materialised_reference_agrees_with_numpy(name):
    """The oracle over the materialised columns against a direct numpy grouping of the evaluated expressions: the
    reference the GPU tests use is itself checked (counts and group keys)."""
    q = parse_sql(CASES[name][0])
    segs = make_table(65)
    ref, _ = R.reference(q, segs)
    assert ref.num_total_docs == sum(s.num_docs for s in segs)
    if q.group_by:
        keys = set()
        for s in segs:
            cols = [R.expr_values(g, s) if isinstance(g, Q.Expr) else R.column_values(s, g) for g in q.group_by]
            mask = np.ones(s.num_docs, bool)
            if q.filter is not None:
                f = q.filter
                v = R.column_values(s, "f")
                mask = (v == 3) if isinstance(f, Q.EqPredicate) else (v >= 10 if f.lower != Q.UNBOUNDED else v < 50)
            keys |= {R.key_bits(tuple(c[i] for c in cols)) for i in np.flatnonzero(mask)}
        assert {R.key_bits(k) for k in ref.groups} == keys
        assert sum(v[[a.function for a in q.aggregations].index("COUNT")] for v in ref.groups.values()) == ref.num_docs_scanned
    assert R.post_filter_entries(q, 10) == 10 * len({c for c in q.columns() if c != "f"})
