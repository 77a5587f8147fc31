"""VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP / COVAR_POP / COVAR_SAMP on the host: parser spellings and result
names, accumulator sharing keys, refusals that need no GPU, reduce.merge_value / final_value against moments_ref.py (the
reference's doc-at-a-time restatement), the count-0 and count-1 defaults, the statistics' column counting, the finish
arithmetic of csrc/pa_moments_finish.h on the host (tests/native/moments_check.cpp under AddressSanitizer +
UndefinedBehaviorSanitizer), and what the pivot is for: the raw power sums in float64 fall outside the bound the GPU
test holds the pivoted ones to."""
import math
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import moments_ref as M
from pinot_amd import parse_sql
from pinot_amd import filter_stats as FS
from pinot_amd import query as Q
from pinot_amd import reduce as R
from pinot_amd import trim as TR
from pinot_amd.engine import CovarianceTuple, VarianceTuple, _empty_value

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ parser
@pytest.mark.parametrize("spelling,function", [
    ("VAR_POP", "VARPOP"), ("var_pop", "VARPOP"), ("VarPop", "VARPOP"), ("VARPOP", "VARPOP"),
    ("VAR_SAMP", "VARSAMP"), ("varsamp", "VARSAMP"), ("STDDEV_POP", "STDDEVPOP"), ("StdDevPop", "STDDEVPOP"),
    ("STD_DEV_POP", "STDDEVPOP"), ("STDDEV_SAMP", "STDDEVSAMP"), ("stddevsamp", "STDDEVSAMP"),
])
def test_variance_spellings(spelling, function):
    q = parse_sql("SELECT %s(x) FROM t" % spelling)  # (fails before the feature: "unsupported aggregation")
    assert q.aggregations == [Q.Aggregation(function, "x")]


@pytest.mark.parametrize("spelling,function", [("COVAR_POP", "COVARPOP"), ("covarpop", "COVARPOP"),
                                               ("CoVar_Samp", "COVARSAMP"), ("COVARSAMP", "COVARSAMP")])
def test_covariance_spellings(spelling, function):
    q = parse_sql("SELECT %s(x, y) FROM t GROUP BY g" % spelling)
    assert q.aggregations == [Q.Aggregation(function, "x", column2="y")]
    assert sorted(q.columns()) == ["g", "x", "y"]


def test_result_column_names():
    """AggregationFunctionType.java:175-187 (covarPop, covarSamp, varPop, varSamp, stdDevPop, stdDevSamp), lower-cased by
    getResultColumnName; the covariance joins its arguments with a comma and no space
    (CovarianceAggregationFunction.java:72-74)."""
    q = parse_sql("SELECT VAR_POP(latency), VAR_SAMP(latency), STDDEV_POP(latency), STDDEV_SAMP(latency), "
                  "COVAR_POP(a, b), COVAR_SAMP(a, b) FROM t")
    assert [a.result_name for a in q.aggregations] == ["varpop(latency)", "varsamp(latency)", "stddevpop(latency)",
                                                       "stddevsamp(latency)", "covarpop(a,b)", "covarsamp(a,b)"]


def test_argument_counts():
    with pytest.raises(ValueError, match="VAR_POP expects 1 argument, got: 2"):
        parse_sql("SELECT VAR_POP(x, y) FROM t")
    with pytest.raises(ValueError, match="STD_DEV_SAMP expects 1 argument, got: 0"):
        parse_sql("SELECT STDDEV_SAMP() FROM t")
    with pytest.raises(ValueError, match="COVARPOP expects 2 arguments, got: 1"):
        parse_sql("SELECT COVAR_POP(x) FROM t")


def test_order_by_and_filter_clause_parse():
    q = parse_sql("SELECT g, STDDEV_POP(x) FROM t GROUP BY g ORDER BY stddev_pop(x) DESC LIMIT 3")
    assert q.order_by[0].expr == q.aggregations[0] and not q.order_by[0].asc
    q = parse_sql("SELECT VAR_POP(x) FILTER (WHERE f < 3), COVAR_POP(x, ADD(y, 1)) FROM t")
    assert q.aggregations[0].filter is not None and isinstance(q.aggregations[1].column2, Q.Expr)
    assert sorted(q.columns()) == ["f", "x", "y"]
    # ORDER BY one of these trims on the host, as FIRST / LASTWITHTIME does
    q = parse_sql("SELECT g, VAR_POP(x) FROM t GROUP BY g ORDER BY g LIMIT 3")
    with pytest.raises(TR.HostTrim):
        TR.lower_order_by(q, [0], False)


def test_statistics_count_each_argument_column_once():
    """StatisticalQueriesTest.java:330: 8 covariances over 6 columns scan NUM_RECORDS * 6 entries after the filter."""
    pairs = [("intColumnX", "intColumnY"), ("doubleColumnX", "doubleColumnY"), ("intColumnX", "doubleColumnX"),
             ("intColumnX", "longColumn"), ("intColumnX", "floatColumn"), ("doubleColumnX", "longColumn"),
             ("doubleColumnX", "floatColumn"), ("longColumn", "floatColumn")]
    q = parse_sql("SELECT %s FROM testTable" % ", ".join("COVAR_POP(%s, %s)" % p for p in pairs))
    assert FS.projected_columns(q) == 6
    assert FS.projected_columns(parse_sql("SELECT VAR_POP(a), STDDEV_SAMP(a), COVAR_SAMP(a, b) FROM t GROUP BY g")) == 3
    assert sorted(Q.query_columns(q)) == sorted({c for p in pairs for c in p})


# ------------------------------------------------------------------ merge / final value
def _segments(rng, sizes, scale=1.0, shift=0.0):
    return [rng.standard_normal(n) * scale + shift for n in sizes]


@pytest.mark.parametrize("sizes", [(1,), (7, 1), (200, 300, 1, 0, 499), (0, 0), (1, 1, 1)])
def test_variance_merge_and_final_follow_the_reference(sizes):
    rng = np.random.default_rng(sum(sizes) + len(sizes))
    segs = _segments(rng, sizes, 500.0, 3.0)
    tuples = [M.variance_segment(s) for s in segs]
    exp = M.variance_table(segs)
    got = VarianceTuple(*tuples[0])
    for t in tuples[1:]:
        got = R.merge_value("VARPOP", got, VarianceTuple(*t))
    assert (got.count, got.sum, got.m2) == exp  # the same operations in the same order: bit for bit
    for fn in Q.VARIANCE_FUNCTIONS:
        a, b = R.final_value(fn, got), M.variance_final(fn, exp)
        assert a == b or (math.isnan(a) and math.isnan(b)), fn
    n, s, m2 = M.exact_variance(np.concatenate(segs).tolist())
    if n > 1:
        assert abs(got.m2 - float(m2)) <= 1e-9 * float(m2)
        assert R.final_value("VARSAMP", got) == got.m2 / (n - 1) and R.final_value("STDDEVPOP", got) == math.sqrt(got.m2 / n)


def test_group_by_path_and_merge():
    rng = np.random.default_rng(5)
    segs = [(rng.integers(0, 4, n).tolist(), rng.standard_normal(n) * 10, rng.standard_normal(n)) for n in (50, 1, 200)]
    exp = M.variance_groups([(k, x) for k, x, _ in segs])
    expc = M.covariance_groups(segs)
    per = [M.variance_groups([(k, x)]) for k, x, _ in segs]
    perc = [M.covariance_groups([s]) for s in segs]
    for key in exp:
        got = gotc = None
        for p, pc in zip(per, perc):
            if key in p:
                t, c = VarianceTuple(*p[key]), CovarianceTuple(*pc[key])
                got = t if got is None else R.merge_value("STDDEVSAMP", got, t)
                gotc = c if gotc is None else R.merge_value("COVARSAMP", gotc, c)
        assert (got.count, got.sum, got.m2) == exp[key]
        assert (gotc.sum_x, gotc.sum_y, gotc.sum_xy, gotc.count) == expc[key]
        for fn in Q.COVARIANCE_FUNCTIONS:
            assert R.final_value(fn, gotc) == M.covariance_final(fn, expc[key])


def test_merge_does_not_change_its_arguments():
    a, b = VarianceTuple(2, 3.0, 0.5), VarianceTuple(3, 9.0, 2.0)
    m = R.merge_value("VARPOP", a, b)
    assert (a, b) == (VarianceTuple(2, 3.0, 0.5), VarianceTuple(3, 9.0, 2.0)) and m.count == 5 and m.sum == 12.0
    assert R.merge_value("VARPOP", a, VarianceTuple(0, 0.0, 0.0)) == a
    assert R.merge_value("VARPOP", VarianceTuple(0, 0.0, 0.0), b) == b
    c = R.merge_value("COVARPOP", CovarianceTuple(1.0, 2.0, 3.0, 4), CovarianceTuple(0.5, 0.25, 1.0, 1))
    assert c == CovarianceTuple(1.5, 2.25, 4.0, 5)


def test_defaults_for_no_doc_and_one_doc():
    """DEFAULT_FINAL_RESULT = -inf for an empty group, and for one doc under the sample forms
    (VarianceAggregationFunction.java:233-240, CovarianceAggregationFunction.java:188-197)."""
    for fn in Q.MOMENT_FUNCTIONS:
        a = Q.Aggregation(fn, "x", column2="y" if fn in Q.COVARIANCE_FUNCTIONS else None)
        empty = _empty_value(a)
        assert empty == (CovarianceTuple(0.0, 0.0, 0.0, 0) if a.column2 else VarianceTuple(0, 0.0, 0.0))
        assert R.final_value(a, empty) == -math.inf and R.final_value(fn, empty) == -math.inf
    one_v, one_c = VarianceTuple(1, 4.0, 0.0), CovarianceTuple(4.0, 2.0, 8.0, 1)
    assert R.final_value("VARSAMP", one_v) == R.final_value("STDDEVSAMP", one_v) == -math.inf
    assert R.final_value("VARPOP", one_v) == R.final_value("STDDEVPOP", one_v) == 0.0
    assert R.final_value("COVARSAMP", one_c) == -math.inf and R.final_value("COVARPOP", one_c) == 0.0


def test_merge_intermediate_and_final_table():
    q = parse_sql("SELECT g, VAR_POP(x), COVAR_SAMP(x, y) FROM t GROUP BY g ORDER BY var_pop(x) DESC LIMIT 10")
    from pinot_amd.engine import IntermediateResult
    parts = []
    for vals in ({(1,): [VarianceTuple(2, 4.0, 2.0), CovarianceTuple(4.0, 2.0, 5.0, 2)]},
                 {(1,): [VarianceTuple(1, 5.0, 0.0), CovarianceTuple(5.0, 1.0, 5.0, 1)],
                  (2,): [VarianceTuple(3, 3.0, 6.0), CovarianceTuple(3.0, 3.0, 9.0, 3)]}):
        r = IntermediateResult(list(q.aggregations), list(q.group_by))
        r.groups = vals
        parts.append(r)
    merged = R.merge_intermediate(parts)
    assert merged.groups[(1,)][0] == R.merge_value("VARPOP", VarianceTuple(2, 4.0, 2.0), VarianceTuple(1, 5.0, 0.0))
    assert merged.groups[(1,)][1] == CovarianceTuple(9.0, 3.0, 10.0, 3)
    table = R.final_result_table(merged, q)
    assert [row[0] for row in table] == [1, 2] or [row[0] for row in table] == [2, 1]
    assert {row[0]: row[1] for row in table}[2] == 2.0


# ------------------------------------------------------------------ the pivot
def test_raw_power_sums_fall_outside_the_bound_the_pivot_keeps():
    """A DOUBLE column of 1e9 + U[0, 10): E[x^2] - E[x]^2 over float64 power sums (what SUM(x), SUM(x * x) gives) misses
    the bound of moments_ref.double_form_bounds, which the pivoted sums of the GPU's double form (restated here in
    numpy float64, in doc order) stay inside — so tests/test_gpu_moments.py can fail."""
    rng = np.random.default_rng(3)
    x = 1e9 + rng.uniform(0, 10, 4000)
    pivot = x.min() / 2 + x.max() / 2
    exact, bound = M.double_form_bounds(x.tolist(), pivot)
    n = len(x)
    s1 = s2 = 0.0
    for v in x.tolist():  # raw power sums, float64
        s1 += v
        s2 += v * v
    raw = s2 - s1 * s1 / n
    assert abs(Fraction(raw) - exact) > bound
    d1 = d2 = 0.0
    for v in x.tolist():  # pivoted, float64
        d = v - pivot
        d1 += d
        d2 += d * d
    piv = math.fma(-d1, d1 / n, d2) if hasattr(math, "fma") else d2 - d1 * (d1 / n)
    assert abs(Fraction(piv) - exact) <= bound
    assert float(bound) < 1e-9 * float(exact)  # (the bound itself is tight: parts in 10^9 of m2)


# ------------------------------------------------------------------ the finish arithmetic on the host
MIN_CASES = {"mul_u64": 200000, "m2_integer": 600000, "covariance_integer": 300000, "double_form": 600000}


def _host_compiler():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    for c in (os.path.join(os.path.dirname(os.path.dirname(hipcc)), "llvm", "bin", "clang++"), shutil.which("g++"),
              shutil.which("c++")):
        if c and os.path.exists(c):
            yield c


def test_finish_arithmetic_matches_int128_on_the_host(tmp_path):
    """tests/native/moments_check.cpp: mul_u64, N = n * S2 - S1^2 and m2 = (double)N / (double)n bit for bit against
    unsigned __int128 (INT32_MIN / INT32_MAX columns up to 2^32 - 1 docs), the integer covariance sums against
    (double)__int128, the double form's fma expressions, n = 0 and NaN; no sanitizer report."""
    exe = str(tmp_path / "moments_check")
    errors = []
    for cxx in _host_compiler():
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
               "-I", os.path.join(ROOT, "pinot_amd", "csrc"), os.path.join(ROOT, "tests", "native", "moments_check.cpp"),
               "-o", exe]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode == 0:
            break
        errors.append("%s: %s" % (cxx, p.stderr[-2000:]))
    else:
        pytest.fail("no host compiler built the check:\n" + "\n".join(errors))
    rep = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert rep.returncode == 0, (rep.stdout[-3000:], rep.stderr[-3000:])
    assert "ERROR" not in rep.stderr and "runtime error" not in rep.stderr and "MISMATCH" not in rep.stderr
    lines = dict((m.group(1), (int(m.group(2)), int(m.group(3)))) for m in
                 re.finditer(r"^(\w+) cases=(\d+) mismatches=(\d+)$", rep.stdout, re.M))
    total = lines.pop("TOTAL")
    assert sorted(lines) == sorted(MIN_CASES)
    for name, (cases, bad) in lines.items():
        assert cases >= MIN_CASES[name] and bad == 0, (name, cases, bad)
    assert total == (sum(c for c, _ in lines.values()), 0)
