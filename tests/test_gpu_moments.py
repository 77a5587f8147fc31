"""VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP / COVAR_POP / COVAR_SAMP on the GPU (the moments scan, STRAT_MOM_LDS =
137 and STRAT_MOM = 138, and the finish kernel of pa_query_fetch_moments) against moments_ref.py: the reference's
doc-at-a-time restatement within the reference test's own relative tolerance, and the exact Fraction evaluator within
bounds derived per form (module docstrings of moments_ref.double_form_bounds and the tests below).

Tables:
  stat  the reference's own shape (StatisticalQueriesTest.java:82-86,183-300): 2,000 rows, 10 groups of 200 consecutive
        rows (a DOUBLE group-by column), values in [-500, 500), four segments of 500 rows with their own dictionaries
  rag   ragged segments of 1, 2,047, 2,049 and 3 x 2,048 + 5 docs and one empty segment, each with its own dictionaries;
        keys g (12 values), u (200 values: most lanes of a step own a key, the ungrouped path, and the block still fits
        LDS), h (about 3,000 values: the block does not fit LDS), c (constant: all 64 lanes of every step on one key, the
        grouped path)
"""
import math
from fractions import Fraction

import numpy as np
import pytest

import moments_ref as M
from pinot_amd import _lib as L
from pinot_amd import parse_sql
from pinot_amd import query as Q
from pinot_amd import reduce as R
from pinot_amd import trim as TR
from pinot_amd.engine import CovarianceTuple, GpuQueryExecutor, GpuSegment, UnsupportedQuery, VarianceTuple
from pinot_amd.segment import create_segment

pytestmark = pytest.mark.gpu

RELATIVE_EPSILON = 1e-4  # StatisticalQueriesTest.java:85
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
# (flags, tuning): both variants, both tile sizes, and a grid of one workgroup so a wave walks several tiles
VARIANTS = {
    "lds16": (L.PA_QF_FORCE_LDS | L.PA_QF_STEPS16, None, "moments_lds"),
    "lds32_grid1": (L.PA_QF_FORCE_LDS | L.PA_QF_STEPS32, {"scan_grid": 1}, "moments_lds"),
    "global16_grid1": (L.PA_QF_FORCE_GLOBAL | L.PA_QF_STEPS16, {"scan_grid": 1}, "moments_global"),
    "global32": (L.PA_QF_FORCE_GLOBAL | L.PA_QF_STEPS32, None, "moments_global"),
}


def close(a, b, eps=RELATIVE_EPSILON):
    """Precision.equalsWithRelativeTolerance: |a - b| <= eps * max(|a|, |b|) (equal infinities are equal)."""
    return a == b or abs(a - b) <= eps * max(abs(a), abs(b))


# ------------------------------------------------------------------ tables
STAT_SCHEMA = {"intColumnX": "INT", "intColumnY": "INT", "doubleColumnX": "DOUBLE", "doubleColumnY": "DOUBLE",
               "longColumn": "LONG", "floatColumn": "FLOAT", "groupByColumn": "DOUBLE"}
STAT_VALUE_COLUMNS = ("intColumnX", "longColumn", "floatColumn", "doubleColumnX")
# StatisticalQueriesTest.java:324-328
STAT_PAIRS = (("intColumnX", "intColumnY"), ("doubleColumnX", "doubleColumnY"), ("intColumnX", "doubleColumnX"),
              ("intColumnX", "longColumn"), ("intColumnX", "floatColumn"), ("doubleColumnX", "longColumn"),
              ("doubleColumnX", "floatColumn"), ("longColumn", "floatColumn"))


@pytest.fixture(scope="module")
def stat():
    rng = np.random.default_rng(20)
    n, groups, mx = 2000, 10, 500
    data = {
        "intColumnX": rng.integers(-mx, mx, n).astype(np.int32), "intColumnY": rng.integers(-mx, mx, n).astype(np.int32),
        "doubleColumnX": rng.uniform(-mx, mx, n), "doubleColumnY": rng.uniform(-mx, mx, n),
        "longColumn": rng.integers(-mx, mx, n).astype(np.int64),
        "floatColumn": (-mx + rng.random(n, dtype=np.float32) * 2 * mx).astype(np.float32),
        "groupByColumn": np.floor(np.arange(n) / (n // groups)),
    }
    datas = [{k: v[i * 500:(i + 1) * 500] for k, v in data.items()} for i in range(4)]
    segs = [create_segment("stat%d" % i, d, STAT_SCHEMA) for i, d in enumerate(datas)]
    gsegs = [GpuSegment(s) for s in segs]
    yield datas, gsegs
    for g in gsegs:
        g.close()


RAG_SCHEMA = {"g": "INT", "u": "INT", "h": "INT", "c": "INT", "f": "INT", "xi": "INT", "xr": "INT", "xl": "LONG", "xw": "LONG",
              "xf": "FLOAT", "xd": "DOUBLE", "dd": "DOUBLE", "mn": "INT", "mx": "INT", "alt": "INT", "nf": "FLOAT",
              "s": "STRING", "rg": "LONG", "mv": "INT"}
RAG_RAW = ("xr", "xl", "xw", "xf", "xd", "mn", "alt", "nf", "rg")
RAG_SIZES = (1, 2047, 2049, 3 * 2048 + 5, 0)
NAN_GROUP = 18  # a value of g (segment seeds differ, so not every segment holds it)


def rag_segment(seed, n):
    rng = np.random.default_rng(seed)
    g = (rng.integers(0, 12, n) * 5 + 3).astype(np.int32)
    nf = rng.standard_normal(n).astype(np.float32) * 100
    nf[(g == NAN_GROUP) & (rng.random(n) < 0.3)] = np.nan
    if n > 5:
        nf[np.flatnonzero(g == NAN_GROUP)[:1]] = np.nan
    data = {
        "g": g, "u": rng.integers(0, 200, n).astype(np.int32), "h": rng.integers(0, 3000, n).astype(np.int32), "c": np.full(n, 42, dtype=np.int32),
        "f": rng.integers(0, 10, n).astype(np.int32),
        "xi": rng.integers(-500 - seed, 500, n).astype(np.int32),                      # dictionary INT
        "xr": rng.integers(INT32_MIN, INT32_MAX + 1, n).astype(np.int32),              # raw INT, the whole range
        "xl": rng.integers(INT32_MIN, INT32_MAX + 1, n).astype(np.int64),              # raw LONG inside int32
        "xw": rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64),                   # raw LONG outside int32
        "xf": (rng.standard_normal(n) * 1e3).astype(np.float32),
        "xd": 1e9 + rng.uniform(0, 10, n),                                              # a large mean, a small spread
        "dd": rng.integers(0, 400 + seed, n) * 1.1 - 50.0,                              # dictionary DOUBLE
        "mn": np.full(n, INT32_MIN, dtype=np.int32), "mx": np.full(n, INT32_MAX, dtype=np.int32),
        "alt": np.where(np.arange(n) % 2 == 0, INT32_MIN, INT32_MAX).astype(np.int32),
        "nf": nf,
        "s": np.array(["ab", "b", "c%d" % seed])[rng.integers(0, 3, n)],
        "rg": rng.integers(0, 50, n).astype(np.int64),
        "mv": [rng.integers(0, 5, size=k).astype(np.int32) for k in rng.integers(1, 3, size=n)],
    }
    return create_segment("rag%d" % seed, data, RAG_SCHEMA, no_dictionary_columns=RAG_RAW, multi_value_columns=("mv",)), data


@pytest.fixture(scope="module")
def rag():
    parts = [rag_segment(31 + i, n) for i, n in enumerate(RAG_SIZES)]
    gsegs = [GpuSegment(s) for s, _ in parts]
    yield [d for _, d in parts], gsegs
    for g in gsegs:
        g.close()


WHERE = {"": lambda d: np.ones(len(d["f"]), dtype=bool), " WHERE f < 3": lambda d: d["f"] < 3,
         " WHERE f > 100": lambda d: d["f"] > 100}


def run(sql, gsegs, flags=0, tuning=None, executions=1, stats=False):
    """-> (result, plan, {aggregation index: (form, pivot)}, section kinds, the executions' results)."""
    ex = GpuQueryExecutor(parse_sql(sql), gsegs, flags=flags, tuning=tuning)
    try:
        results = []
        for _ in range(executions):
            ex.execute()
            results.append(ex.fetch(execution_stats=stats))
        plan = ex.stats()["plan"]
        forms = {ai: plan["moments_form"][pi] for ai, pi in enumerate(ex.agg_map) if pi in plan["moments_form"]}
        return results[-1], plan, forms, [kind for kind, _, _ in ex.sections()], results
    finally:
        ex.close()


def rows_of(res, query):
    """{key (None for an aggregation-only query): [intermediate value per aggregation]}."""
    if not query.group_by:
        return {None: list(res.row)}
    return {k[0]: list(v) for k, v in res.groups.items()}


def group_docs(datas, key, where, limit=None):
    """{key: [(segment, doc index array)]} of the matching docs, in segment order; `limit`: the numGroupsLimit prefix walk
    (a segment admits the first `limit` distinct keys of its matching docs in docId order)."""
    out = {}
    for si, d in enumerate(datas):
        mask = WHERE[where](d)
        if key is None:
            out.setdefault(None, []).append((si, np.flatnonzero(mask)))
            continue
        keys = d[key]
        admitted = None
        if limit is not None:
            admitted = []
            for k in keys[mask].tolist():
                if k not in admitted:
                    if len(admitted) == limit:
                        continue
                    admitted.append(k)
        for k in np.unique(keys[mask]).tolist():
            if admitted is not None and k not in admitted:
                continue
            out.setdefault(k, []).append((si, np.flatnonzero(mask & (keys == k))))
    return out


def values_of(datas, parts, column):
    return np.concatenate([datas[si][column][idx] for si, idx in parts]) if parts else np.zeros(0)


# references over the module's tables (the restatement's tuples, exact values, bounds), computed once and shared by the
# variants that need them; never changed afterwards
_ONCE = {}


def once(memo, compute):
    if memo not in _ONCE:
        _ONCE[memo] = compute()
    return _ONCE[memo]


def docs_of(datas, key, where, limit=None):
    return once(("docs", key, where, limit), lambda: group_docs(datas, key, where, limit))


# ------------------------------------------------------------------ the reference's own shape
@pytest.mark.parametrize("shape,variant", [("all", "lds16"), ("all", "global32"), ("filtered", "lds32_grid1"),
                                           ("filtered", "global16_grid1"), ("group_by", ""), ("group_by", "global32")])
def test_reference_shape(stat, shape, variant):
    """Aggregation-only, filtered (groupByColumn < 5) and GROUP BY over INT, LONG, FLOAT and DOUBLE arguments and the mixed
    covariance pairs of StatisticalQueriesTest.java:324-328: every intermediate tuple and every final value against the
    doc-at-a-time restatement within RELATIVE_EPSILON, and the execution statistics (:330: the distinct argument columns,
    each once, plus the group-by column)."""
    datas, gsegs = stat
    flags, tuning, _ = VARIANTS[variant] if variant else (0, None, None)
    sel = ["%s(%s)" % (fn, c) for c in STAT_VALUE_COLUMNS for fn in ("VAR_POP", "VAR_SAMP", "STDDEV_POP", "STDDEV_SAMP")]
    sel += ["%s(%s, %s)" % (fn, x, y) for x, y in STAT_PAIRS for fn in ("COVAR_POP", "COVAR_SAMP")]
    where = " WHERE groupByColumn < 5" if shape == "filtered" else ""
    sql = "SELECT %s%s FROM t%s%s LIMIT 1000" % ("groupByColumn, " if shape == "group_by" else "", ", ".join(sel), where,
                                                 " GROUP BY groupByColumn" if shape == "group_by" else "")
    query = parse_sql(sql)
    stats = "global" not in variant  # (the statistics do not depend on the variant: asked for once per shape)
    res, plan, forms, _, _ = run(sql, gsegs, flags, tuning, stats=stats)
    assert plan["strategy"] == "moments"
    masks = [d["groupByColumn"] < 5 if shape == "filtered" else np.ones(500, dtype=bool) for d in datas]
    docs = int(sum(m.sum() for m in masks))
    assert (res.num_docs_scanned, res.num_total_docs) == (docs, 2000)
    if stats:
        assert res.num_entries_scanned_post_filter == docs * (7 if shape == "group_by" else 6)
    got = rows_of(res, query)
    assert len(got) == (10 if shape == "group_by" else 1)
    for ai, a in enumerate(query.aggregations):
        if a.function in Q.VARIANCE_FUNCTIONS:
            if shape == "group_by":
                exp = once(("stat", shape, a.column), lambda: M.variance_groups(
                    [(d["groupByColumn"][m].tolist(), d[a.column][m]) for d, m in zip(datas, masks)]))
            else:
                exp = once(("stat", shape, a.column),
                           lambda: {None: M.variance_table([d[a.column][m] for d, m in zip(datas, masks)])})
            for k, e in exp.items():
                t = got[k][ai]
                assert isinstance(t, VarianceTuple) and t.count == e[0], (a.result_name, k)
                assert close(t.sum, e[1]) and close(t.m2, e[2]), (a.result_name, k, t, e)
                assert close(R.final_value(a, t), M.variance_final(a.function, e)), (a.result_name, k, t, e)
        else:
            if shape == "group_by":
                exp = once(("stat", shape, a.column, a.column2), lambda: M.covariance_groups(
                    [(d["groupByColumn"][m].tolist(), d[a.column][m], d[a.column2][m]) for d, m in zip(datas, masks)]))
            else:
                exp = once(("stat", shape, a.column, a.column2), lambda: {None: M.covariance_table(
                    [(d[a.column][m], d[a.column2][m]) for d, m in zip(datas, masks)])})
            for k, e in exp.items():
                t = got[k][ai]
                assert isinstance(t, CovarianceTuple) and t.count == e[3], (a.result_name, k)
                assert close(t.sum_x, e[0]) and close(t.sum_y, e[1]) and close(t.sum_xy, e[2]), (a.result_name, k, t, e)
                assert close(R.final_value(a, t), M.covariance_final(a.function, e)), (a.result_name, k, t, e)
    # INT / LONG arguments (pairs of them) keep exact integers; everything else doubles
    integer = {"intColumnX", "intColumnY", "longColumn"}
    for ai, a in enumerate(query.aggregations):
        cols = {a.column} | ({a.column2} if a.column2 else set())
        assert forms[ai][0] == (L.PA_MOMENTS_FORM_INTEGER if cols <= integer else L.PA_MOMENTS_FORM_DOUBLE), a.result_name


# ------------------------------------------------------------------ integer form: exactness
INT_COLUMNS = ("xi", "xr", "xl", "mn", "mx", "alt")
INT_PAIRS = (("xr", "alt"), ("mn", "mx"), ("mn", "mn"), ("xi", "xl"))


def check_integer(datas, query, res, forms, where, limit=None):
    key = query.group_by[0] if query.group_by else None
    docs = docs_of(datas, key, where, limit)
    got = rows_of(res, query)
    if key is not None:
        assert sorted(got) == sorted(docs)
    for ai, a in enumerate(query.aggregations):
        if a.function not in Q.MOMENT_FUNCTIONS:
            continue
        assert forms[ai] == (L.PA_MOMENTS_FORM_INTEGER, 0.0), a.result_name
        for k, parts in docs.items():
            t = got[k][ai]
            if a.function in Q.VARIANCE_FUNCTIONS:
                n, s, m2 = once(("exact", key, where, limit, k, a.column),
                                lambda: M.exact_variance(values_of(datas, parts, a.column).tolist()))
                # count and sum exactly (|sum| < 2^53 here); m2 = (double)N / (double)n with N exact: the conversion of N
                # (at most two roundings), and one division: (1 + 2^-53)^3 - 1 < 2^-51 relative
                assert (t.count, Fraction(t.sum)) == (n, s), (a.result_name, k)
                assert abs(Fraction(t.m2) - m2) <= m2 * Fraction(1, 1 << 51), (a.result_name, k, t.m2, float(m2))
            else:
                sx, sy, sxy, n = once(("exact", key, where, limit, k, a.column, a.column2),
                                      lambda: M.exact_covariance(values_of(datas, parts, a.column).tolist(),
                                                                 values_of(datas, parts, a.column2).tolist()))
                # the correctly rounded doubles of the exact integers (the sums of x and y are below 2^53: exact)
                assert (t.count, Fraction(t.sum_x), Fraction(t.sum_y), t.sum_xy) == (n, sx, sy, M.nearest_double(sxy)), \
                    (a.result_name, k, t)


# every key shape on an LDS and on a device-scope variant, every variant on a grouped and on an ungrouped key shape
INTEGER_CASES = [(None, "lds16"), (None, "global32"), ("g", "lds32_grid1"), ("g", "global16_grid1"), ("u", "lds16"),
                 ("u", "global32"), ("h", "global16_grid1"), ("c", "lds32_grid1"), ("c", "global32")]


@pytest.mark.parametrize("key,variant", INTEGER_CASES)
def test_integer_form_is_exact_and_deterministic(rag, key, variant):
    """INT32_MIN / INT32_MAX / alternating columns (6,149 docs of INT32_MIN in one segment: the sum of squares passes
    2^64, the pair carries; products of -2^31 * (2^31 - 1)), a raw INT column over the whole range and a LONG column
    inside int32; all 64 lanes on one key (c), about 64 keys per step (u, h; the accumulators of h's 3,000 keys do not fit
    LDS: the planner takes the device-scope variant whatever the flag); both variants and tile sizes; a filter; two
    executions of one executor agree bit for bit with each other and with the other variant's of the same key shape (the
    first case of a key shape keeps its rows, the second compares with them)."""
    datas, gsegs = rag
    flags, tuning, name = VARIANTS[variant]
    sel = ", ".join(["VAR_POP(%s)" % c for c in INT_COLUMNS] + ["COVAR_POP(%s, %s)" % p for p in INT_PAIRS] +
                    ["COUNT(*)", "SUM(xi)"])
    for where in ("", " WHERE f < 3"):
        sql = "SELECT %s%s FROM t%s%s LIMIT 100000" % (key + ", " if key else "", sel, where, " GROUP BY " + key if key else "")
        res, plan, forms, kinds, results = run(sql, gsegs, flags, tuning, executions=2)
        assert plan["variant"] == (name if key != "h" else "moments_global") and plan["steps"] == (16 if "16" in variant else 32)
        assert kinds.count(L.PA_ACC_MOM_I64) == len(INT_COLUMNS) + len(INT_PAIRS) and L.PA_ACC_MOM_F64 not in kinds
        query = parse_sql(sql)
        check_integer(datas, query, res, forms, where)
        a, b = (rows_of(r, query) for r in results)
        assert a == b  # (dataclass equality of the doubles: bit for bit, no NaN here)
        assert once(("integer rows", key, where), lambda: a) == a


def test_integer_and_double_forms_in_one_query(rag):
    """A LONG column inside int32 (integer form) next to one outside (double form), with ordinary aggregations."""
    datas, gsegs = rag
    sql = "SELECT g, STDDEV_SAMP(xl), STDDEV_SAMP(xw), VAR_SAMP(xl), MAX(xw), COUNT(*) FROM t GROUP BY g LIMIT 1000"
    res, plan, forms, kinds, _ = run(sql, gsegs)
    assert forms[0][0] == forms[2][0] == L.PA_MOMENTS_FORM_INTEGER and forms[1][0] == L.PA_MOMENTS_FORM_DOUBLE
    assert kinds.count(L.PA_ACC_MOM_I64) == 1 and kinds.count(L.PA_ACC_MOM_F64) == 1  # (xl's two spellings share one)
    query = parse_sql(sql)
    docs = docs_of(datas, "g", "")
    for k, row in rows_of(res, query).items():
        n, s, m2 = once(("exact", "g", "", None, k, "xl"), lambda: M.exact_variance(values_of(datas, docs[k], "xl").tolist()))
        assert (row[0].count, Fraction(row[0].sum)) == (n, s) and row[0] == row[2]
        assert abs(Fraction(row[0].m2) - m2) <= m2 * Fraction(1, 1 << 51)
        em2, bound = M.double_form_bounds(values_of(datas, docs[k], "xw").tolist(), forms[1][1])
        assert abs(Fraction(row[1].m2) - em2) <= bound
        assert row[3] == float(values_of(datas, docs[k], "xw").max()) and row[4] == n


# ------------------------------------------------------------------ double form: a-priori bounds
DOUBLE_COLUMNS = ("xd", "xf", "xw", "dd")


@pytest.mark.parametrize("key,variant", [(None, "lds16"), ("g", "lds32_grid1"), ("g", "global32"), ("c", "global16_grid1")])
def test_double_form_within_the_summation_bound(rag, key, variant):
    """Per group |m2 - m2_exact| <= the bound of moments_ref.double_form_bounds, computed from that group's own pivoted
    values with the pivot the library reports (no fixed relative tolerance); the sum within the same kind of bound. xd =
    1e9 + U[0, 10): the pivot is what keeps the result inside (tests/test_moments.py shows the raw power sums outside)."""
    datas, gsegs = rag
    flags, tuning, name = VARIANTS[variant]
    sel = ", ".join("VAR_POP(%s)" % c for c in DOUBLE_COLUMNS)
    sql = "SELECT %s%s FROM t WHERE f < 7%s LIMIT 1000" % (key + ", " if key else "", sel, " GROUP BY " + key if key else "")
    WHERE[" WHERE f < 7"] = lambda d: d["f"] < 7
    res, plan, forms, kinds, _ = run(sql, gsegs, flags, tuning)
    assert plan["variant"] == name and kinds.count(L.PA_ACC_MOM_F64) == len(DOUBLE_COLUMNS)
    query = parse_sql(sql)
    docs = docs_of(datas, key, " WHERE f < 7")
    got = rows_of(res, query)
    assert sorted(got, key=str) == sorted(docs, key=str)
    for ai, c in enumerate(DOUBLE_COLUMNS):
        form, pivot = forms[ai]
        assert form == L.PA_MOMENTS_FORM_DOUBLE and math.isfinite(pivot)
        allv = np.concatenate([d[c] for d in datas]).astype(np.float64)
        assert pivot == allv.min() / 2 + allv.max() / 2, c
        for k, parts in docs.items():
            n, em2, bound, exact_sum, sb = once(("double", key, k, c, pivot), lambda: M.double_form_bounds(
                values_of(datas, parts, c).tolist(), pivot, with_sum=True))
            t = got[k][ai]
            assert t.count == n
            assert abs(Fraction(t.m2) - em2) <= bound, (c, k, t.m2, float(em2), float(bound))
            # sum = fma(n, pivot, S1): S1 within its summation bound, one more rounding of the result
            assert abs(Fraction(t.sum) - exact_sum) <= sb + (abs(exact_sum) + sb) * Fraction(1, 1 << 53), (c, k)


@pytest.mark.parametrize("variant", ["lds32_grid1", "global16_grid1"])
def test_double_form_covariance_sums(rag, variant):
    """Covariance in the double form keeps the reference's raw sums: each of the three against the summation bound of its
    own terms (a mixed INT x DOUBLE pair, a FLOAT x DOUBLE pair, a LONG outside int32 with a dictionary DOUBLE)."""
    datas, gsegs = rag
    flags, tuning, _ = VARIANTS[variant]
    pairs = (("xi", "xd"), ("xf", "xd"), ("xw", "dd"))
    sql = "SELECT g, %s FROM t GROUP BY g LIMIT 1000" % ", ".join("COVAR_SAMP(%s, %s)" % p for p in pairs)
    res, _, forms, _, _ = run(sql, gsegs, flags, tuning)
    docs = docs_of(datas, "g", "")
    got = rows_of(res, parse_sql(sql))

    def bounds(parts, x, y):
        xs = [M.frac(v) for v in values_of(datas, parts, x).tolist()]
        ys = [M.frac(v) for v in values_of(datas, parts, y).tolist()]
        return len(xs), [M.sum_bound(terms) for terms in (xs, ys, [a * b for a, b in zip(xs, ys)])]

    for ai, (x, y) in enumerate(pairs):
        assert forms[ai] == (L.PA_MOMENTS_FORM_DOUBLE, 0.0)
        for k, parts in docs.items():
            n, sums = once(("covariance sums", k, x, y), lambda: bounds(parts, x, y))
            t = got[k][ai]
            assert t.count == n
            for value, (exact, bound) in zip((t.sum_x, t.sum_y, t.sum_xy), sums):
                assert abs(Fraction(value) - exact) <= bound, (x, y, k)


def test_nan_stays_in_its_group(rag):
    """NaN in a FLOAT column: NaN for the groups holding one, the other groups inside their bound; the pivot ignores it."""
    datas, gsegs = rag
    sql = "SELECT g, VAR_POP(nf), STDDEV_POP(nf) FROM t GROUP BY g LIMIT 1000"
    for variant in ("lds16", "global32"):
        res, _, forms, _, _ = run(sql, gsegs, *VARIANTS[variant][:2])
        pivot = forms[0][1]
        assert math.isfinite(pivot)
        docs = docs_of(datas, "g", "")
        got = rows_of(res, parse_sql(sql))
        seen_nan = 0
        for k, parts in docs.items():
            vals = values_of(datas, parts, "nf")
            if np.isnan(vals).any():
                seen_nan += 1
                assert math.isnan(got[k][0].m2) and math.isnan(R.final_value("STDDEVPOP", got[k][1])), k
            else:
                em2, bound = once(("nan", k, pivot), lambda: M.double_form_bounds(vals.tolist(), pivot))
                assert abs(Fraction(got[k][0].m2) - em2) <= bound, k
        assert seen_nan == 1 and len(docs) == 12


# ------------------------------------------------------------------ other
def test_num_groups_limit_walk(rag):
    """numGroupsLimit below the number of groups: every segment admits its first 50 keys (the prefix walk) and the moment
    sums are those of the admitted keys' docs."""
    datas, gsegs = rag
    sql = "SELECT h, VAR_POP(xr), COVAR_POP(xr, alt), COUNT(*) FROM t%s GROUP BY h LIMIT 100000 OPTION(numGroupsLimit=50)"
    for where in ("", " WHERE f < 3"):
        res, plan, forms, _, _ = run(sql % where, gsegs)
        assert plan["limit_trimming"] == 2 and res.num_groups_limit_reached
        check_integer(datas, parse_sql(sql % where), res, forms, where, limit=50)


def test_filter_matching_nothing(rag):
    _, gsegs = rag
    res, _, _, _, _ = run("SELECT VAR_POP(xi), STDDEV_SAMP(xd), COVAR_POP(xi, xd) FROM t WHERE f > 100", gsegs)
    assert list(res.row) == [VarianceTuple(0, 0.0, 0.0), VarianceTuple(0, 0.0, 0.0), CovarianceTuple(0.0, 0.0, 0.0, 0)]
    assert [R.final_value(a, v) for a, v in zip(res.aggregations, res.row)] == [-math.inf] * 3
    res, _, _, _, _ = run("SELECT g, VAR_POP(xi) FROM t WHERE f > 100 GROUP BY g", gsegs)
    assert res.groups == {}


def test_server_trim_falls_back_to_the_host(rag):
    _, gsegs = rag
    q = parse_sql("SELECT h, STDDEV_POP(xi) FROM t GROUP BY h ORDER BY stddev_pop(xi) DESC LIMIT 3 "
                  "OPTION(minServerGroupTrimSize=10)")
    ex = GpuQueryExecutor(q, gsegs)
    try:
        ex.execute()
        trimmed = ex.fetch(execution_stats=False, server_trim=True)
        assert ex.last_trim["device"] is False and ex.last_trim["kept"] == 15 < ex.last_trim["groups"]
        full = ex.fetch(execution_stats=False)
        assert trimmed.groups == R.server_trim(full, ex.query).groups
        assert len(R.final_result_table(trimmed, ex.query)) == 3
        with pytest.raises(L.PinotAmdError) as e:  # the library itself refuses the device trim of such a query
            ex.fetch_arrays(trim_spec=TR.build_spec([(L.PA_TRIM_COUNT, 0, 0, 0)], 5))
        assert e.value.code == L.PA_EUNSUPPORTED
    finally:
        ex.close()


@pytest.mark.parametrize("sql,reason", [
    ("SELECT rg, VAR_POP(xi) FROM t GROUP BY rg", "hashed key space"),                          # raw group-by column
    ("SELECT g, VAR_POP(xr) FROM t GROUP BY g, h, xi, dd", "hashed key space"),                 # too large to address
    ("SELECT VAR_POP(xi) FROM t GROUP BY ADD(xi, 1)", "transform expressions"),                 # expression key
    ("SELECT mv, VAR_POP(xi) FROM t GROUP BY mv", "multi-value"),                               # MV group-by column
    ("SELECT VAR_POP(xi), SUMMV(mv) FROM t", "multi-value"),                                    # MV aggregation column
    ("SELECT STDDEV_POP(mv) FROM t", "multi-value column mv"),
    ("SELECT COVAR_POP(xi, mv) FROM t", "multi-value column mv"),
    ("SELECT VAR_SAMP(ADD(xi, 1)) FROM t", "transform expression as its argument"),
    ("SELECT COVAR_SAMP(xi, xi * 2) FROM t", "transform expression as its argument"),
    ("SELECT VAR_POP(s) FROM t", "over the STRING column s"),
    ("SELECT VAR_POP(xi) FILTER (WHERE f < 3) FROM t", "FILTER"),
    ("SELECT VAR_POP(xi), SUM(xi) FILTER (WHERE f < 3) FROM t", "aggregation filters"),
    ("SELECT VAR_POP(xi) FROM t OPTION(enableNullHandling=true)", "null handling"),
    ("SELECT h, VAR_POP(xi) FROM t GROUP BY h OPTION(numGroupsLimit=50)", "first-position"),
    ("SELECT VAR_POP(xi), SUM(ADD(xi, 1)) FROM t", "transform expressions"),
])
def test_refusals(rag, sql, reason):
    _, gsegs = rag
    flags = L.PA_QF_NO_LIMIT_WALK if "numGroupsLimit" in sql else 0
    with pytest.raises(UnsupportedQuery, match=reason):
        GpuQueryExecutor(parse_sql(sql), gsegs, flags=flags).close()


def test_forced_forms_and_pivot(rag):
    """pa_query_set_moments: the agreed form and pivot of a multi-GPU query reach the library and decide the sections; the
    integer form on a column outside int32 is an error."""
    datas, gsegs = rag
    q = parse_sql("SELECT VAR_POP(xl), VAR_POP(xd) FROM t")
    ex = GpuQueryExecutor(q, gsegs, moments={("xl", None): (L.PA_MOMENTS_FORM_DOUBLE, 12.5),
                                             ("xd", None): (L.PA_MOMENTS_FORM_AUTO, 1e9)})
    try:
        assert ex.moments_form(0) == (L.PA_MOMENTS_FORM_DOUBLE, 12.5) and ex.moments_form(1) == (L.PA_MOMENTS_FORM_DOUBLE, 1e9)
        ex.execute()
        res = ex.fetch(execution_stats=False)
        for t, c, pivot in zip(res.row, ("xl", "xd"), (12.5, 1e9)):
            em2, bound = M.double_form_bounds(np.concatenate([d[c] for d in datas]).tolist(), pivot)
            assert abs(Fraction(t.m2) - em2) <= bound
    finally:
        ex.close()
    with pytest.raises(L.PinotAmdError, match="integer form"):
        GpuQueryExecutor(parse_sql("SELECT VAR_POP(xw) FROM t"), gsegs,
                         moments={("xw", None): (L.PA_MOMENTS_FORM_INTEGER, None)}).close()
