"""Selection queries on the GPU (engine.SelectionExecutor: the fused filter + top-K scan, the finish kernels, the cell
gather) against the numpy restatement tests/selection_ref.py. Equality is exact — (segment, doc, key, values) of every
row — because ties break by (segment, doc), which makes the result unique. The golden cases are the reference's own
(tests/golden/sv_selection.json); the synthetic shapes are the ones at which the kernel can go wrong: ragged tiles, a
one-doc segment, per-segment dictionaries, several tiles per wave, K inside a tie group, a 0-bit key component, a
64-bit key, all-ones keys, compaction of a full candidate segment."""
import ctypes
import json
import os

import numpy as np
import pytest

import selection_ref as R
from conftest import GOLDEN
from pinot_amd import _lib as L
from pinot_amd import parse_sql
from pinot_amd.segment import create_segment
from test_selection import case_sql, check_golden_case

pytestmark = pytest.mark.gpu

HI, LO = "\uffff", "\U00010000"  # String.compareTo: LO < HI (UTF-16 code units); by code point HI < LO
BIG = 777777                      # the frequent value of column u in the largest segment


def _norm(rows):
    return [[repr(v) if isinstance(v, float) else v for v in r] for r in rows]


def run_gpu(gsegs, query, tuning=None):
    """(SelectionResult, counters or None, eager literals or None) of one query over resident segments."""
    from pinot_amd.engine import SelectionExecutor
    ex = SelectionExecutor(query, gsegs, tuning=tuning)
    try:
        res = ex.run()
        if ex.handle is None:
            return res, None, None
        return res, ex.counters(), int(L.lib().pa_query_num_eager_literals(ex.handle))
    finally:
        ex.close()


def assert_same(got, ref, k):
    """The GPU result against the first k rows of the restatement's full order."""
    n = min(k, len(ref.rows))
    assert len(got.rows) == n
    assert list(got.columns) == list(ref.columns)
    assert got.segments.tolist() == ref.segments[:n].tolist()
    assert got.docs.tolist() == ref.docs[:n].tolist()
    assert got.keys.tolist() == ref.keys[:n].tolist()
    assert _norm(got.rows) == _norm(ref.rows[:n])


# ------------------------------------------------------------------ golden cases
@pytest.fixture(scope="module")
def golden_gpu(golden_segment):
    from pinot_amd.engine import GpuSegment
    g = GpuSegment(golden_segment, device=0)
    yield g
    g.close()


def test_golden_selection_cases(golden_gpu, golden_segment):
    """Every case of InnerSegmentSelectionSingleValueQueriesTest the fixture holds: the asserted rows and schema, the
    four statistics where the reference runs SelectionOrderByOperator, and the whole result against the restatement."""
    with open(os.path.join(GOLDEN, "sv_selection.json")) as f:
        spec = json.load(f)
    for case in spec["cases"]:
        q = parse_sql(case_sql(spec, case))
        got, _, _ = run_gpu([golden_gpu], q)
        stats = [got.num_docs_scanned, got.num_entries_scanned_in_filter, got.num_entries_scanned_post_filter,
                 got.num_total_docs]
        if case["stats"] is None:
            # column5 / daysSinceEpoch are sorted in this segment and no ORDER BY stops early: not modelled
            assert stats[:3] == [None, None, None], case["source"]
        check_golden_case(case, got, q, stats)
        for name, t in case.get("types", {}).items():
            assert got.column_types[got.columns.index(name)] == t
        if "schema_types" in case:
            assert got.column_types == case["schema_types"]
        if q.offset + q.limit:
            assert_same(got, R.run(q, [golden_segment]), q.offset + q.limit)


# ------------------------------------------------------------------ synthetic shapes
def _segments():
    rng = np.random.default_rng(20261)
    out = []
    for si, n in enumerate((1, 2049, 20001)):
        pool = np.array(["s%03d" % i for i in range((1, 9, 150)[si])] + ([HI, "zz" + LO] if si == 1 else [LO, HI + "a"]))
        i64 = np.iinfo(np.int64)
        data = {
            "two": rng.integers(0, 2, n).astype(np.int32),
            "one": np.full(n, 42, dtype=np.int32),
            "a": (rng.integers(0, (1, 37, 700)[si], n) * 3 + si).astype(np.int32),
            "b": rng.integers(0, (1, 100, 5000)[si], n).astype(np.int64) * 1000003 - (1 << 40),
            "c": rng.integers(-300, (1, 50, 900)[si], n).astype(np.float64) / 8,
            "s": pool[rng.integers(0, len(pool), n)],
            "f": rng.integers(0, 50, n).astype(np.int32),
            "u": (np.arange(n) + 1000000).astype(np.int32),
            "ri": rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32),
            "rl": rng.integers(i64.min, i64.max, n, dtype=np.int64),
            "rf": rng.normal(0, 100, n).astype(np.float32),
            "rd": rng.normal(0, 1e6, n).astype(np.float64),
        }
        if n > 100:
            # extremes and special values, each more than once (ties) and next to ordinary values
            at = rng.choice(n, 40, replace=False)
            data["ri"][at[:4]] = [-(1 << 31), (1 << 31) - 1, -(1 << 31), (1 << 31) - 1]
            data["rl"][at[4:8]] = [i64.min, i64.max, i64.min, i64.max]
            data["rf"][at[8:18]] = [0.0, -0.0, np.inf, -np.inf, np.nan, 0.0, -0.0, np.inf, -np.inf, np.nan]
            data["rd"][at[18:28]] = [0.0, -0.0, np.inf, -np.inf, np.nan, 0.0, -0.0, np.inf, -np.inf, -np.nan]
        if n == 20001:
            # 16400 distinct values and one frequent one: an equality on it is estimated sparse (one dictId of 16401),
            # so the planner evaluates the other clauses lazily, yet it matches 3601 docs
            data["u"][16400:] = BIG
        schema = {"two": "INT", "one": "INT", "a": "INT", "b": "LONG", "c": "DOUBLE", "s": "STRING", "f": "INT",
                  "u": "INT", "ri": "INT", "rl": "LONG", "rf": "FLOAT", "rd": "DOUBLE"}
        out.append(create_segment("syn%d" % si, data, schema, no_dictionary_columns=("ri", "rl", "rf", "rd")))
    return out


@pytest.fixture(scope="module")
def synth():
    from pinot_amd.engine import GpuSegment
    segs = _segments()
    gsegs = [GpuSegment(s, device=0) for s in segs]
    yield segs, gsegs
    for g in gsegs:
        g.close()


FILTERS = {
    "none": "",
    "eager_range": " WHERE f BETWEEN 10 AND 30",
    # eager equality (estimated sparse) + lazy clauses, one of them on the ORDER BY column a
    "eager_and_lazy": " WHERE u = %d AND a > 600 AND ri > -1500000000" % BIG,
    "matches_nothing": " WHERE f > 1000",
}
ORDERS = {
    "two_values": "two",                       # K cuts inside a tie group that spans segments
    "zero_bit_component": "one, a",            # a dictionary of one value: a 0-bit key component
    "three_mixed": "a DESC, b, c DESC",
    "three_mixed_2": "c, a DESC, s",
    "string": "s DESC",
    "raw_int": "ri",
    "raw_long_desc": "rl DESC",                # INT64_MIN DESC: an all-ones key
    "raw_long": "rl",
    "raw_float": "rf",
    "raw_double_desc": "rd DESC",
    "key_of_64_bits": "ri DESC, rf",           # 32 + 32 bits
    "dict_and_raw": "two DESC, rf DESC, a",    # 1 + 32 + 10 bits
}


@pytest.mark.parametrize("order", list(ORDERS))
def test_synthetic_shapes(synth, order):
    """3 segments of 1, 2049 and 20001 docs with their own dictionaries, one workgroup (4 waves, several tiles each),
    every filter shape, K in {1, 10, 64, matched - 1, matched, matched + 5, all docs}."""
    segs, gsegs = synth
    total = sum(s.num_docs for s in segs)
    for fname, where in FILTERS.items():
        base = "SELECT s, rl, a FROM t%s ORDER BY %s" % (where, ORDERS[order])
        ref = R.run(parse_sql(base + " LIMIT %d" % total), segs)
        m = ref.matched
        assert (m == 0) == (fname == "matches_nothing")
        for k in sorted({k for k in (1, 10, 64, m - 1, m, m + 5, total) if 1 <= k <= total}):
            q = parse_sql(base + " LIMIT %d" % k)
            got, counters, eager = run_gpu(gsegs, q, tuning={"scan_grid": 1})
            assert_same(got, ref, k)
            assert counters["waves"] == 4
            if fname == "eager_and_lazy":
                assert eager == 1  # the other clauses ran per surviving doc
            if order != "zero_bit_component":  # (column `one` is sorted: the reference would stop early)
                assert got.num_docs_scanned == m
                nob = len({o.expr for o in q.order_by})
                exp_post = m * nob + sum(min(k, x) for x in ref.segment_matched) * (len(ref.columns) - nob)
                assert got.num_entries_scanned_post_filter == exp_post
            else:
                assert got.num_docs_scanned is None


def test_no_order_by_is_the_first_matching_docs(synth):
    segs, gsegs = synth
    for where in FILTERS.values():
        q = parse_sql("SELECT * FROM t%s LIMIT 3000" % where)
        got, _, _ = run_gpu(gsegs, q, tuning={"scan_grid": 1})
        assert_same(got, R.run(q, segs), 3000)
        assert set(got.keys.tolist()) <= {0} and got.num_docs_scanned is None


# ------------------------------------------------------------------ compaction
@pytest.mark.parametrize("shape", ["monotone_improving", "random"])
def test_compaction_of_full_candidate_segments(shape):
    """Every doc beats the wave's bound (values ascending in doc order under ORDER BY ... DESC), so the candidate
    segments fill and compact over and over; a random order fills them a few times. CAP = K + 1 and 2 K."""
    from pinot_amd.engine import GpuSegment
    rng = np.random.default_rng(5)
    segs = []
    for si, n in enumerate((3000, 9001)):
        v = np.sort(rng.integers(0, 1 << 20, n)) if shape == "monotone_improving" else rng.integers(0, 1 << 20, n)
        data = {"v": v.astype(np.int32), "w": rng.integers(0, 5, n).astype(np.int32), "r": v.astype(np.int64) * 7 - 11}
        segs.append(create_segment("cmp%d" % si, data, {"v": "INT", "w": "INT", "r": "LONG"}, no_dictionary_columns=("r",)))
    gsegs = [GpuSegment(s, device=0) for s in segs]
    try:
        for order in ("v DESC", "r DESC"):
            for k in (10, 100):
                q = parse_sql("SELECT w, v FROM t ORDER BY %s LIMIT %d" % (order, k))
                ref = R.run(q, segs)
                for cap in (k + 1, 2 * k):
                    got, counters, _ = run_gpu(gsegs, q, tuning={"scan_grid": 1, "select_cap": cap})
                    assert_same(got, ref, k)
                    assert counters["cap"] == cap and counters["waves"] > 1
                    assert counters["compactions"] > 0
                    assert counters["appended"] >= k
    finally:
        for g in gsegs:
            g.close()


# ------------------------------------------------------------------ refusals
def test_refusals(synth):
    from pinot_amd.engine import GpuSegment, SelectionExecutor, UnsupportedQuery
    segs, gsegs = synth
    with pytest.raises(UnsupportedQuery, match="64 bits"):
        SelectionExecutor(parse_sql("SELECT a FROM t ORDER BY rl, rd LIMIT 5"), gsegs)
    with pytest.raises(UnsupportedQuery, match="PA_MAX_SELECT_ROWS"):
        SelectionExecutor(parse_sql("SELECT a FROM t ORDER BY a LIMIT 65537"), gsegs)
    mv = create_segment("mv", {"m": [np.array([1, 2]), np.array([3])], "x": np.array([5, 6], dtype=np.int32)},
                        {"m": "INT", "x": "INT"}, multi_value_columns=("m",))
    g = GpuSegment(mv, device=0)
    try:
        with pytest.raises(UnsupportedQuery, match="multi-value"):
            SelectionExecutor(parse_sql("SELECT m FROM t ORDER BY x LIMIT 5"), [g])
        # the C-ABI refuses it too, whatever the host checked
        lib = L.lib()
        spec = L.QuerySpec()
        spec.num_aggs = 1
        spec.aggs[0].type = L.PA_AGG_COUNT
        h = L.check_ptr(lib.pa_query_create(ctypes.byref(spec), 1), "pa_query_create")
        try:
            sel = L.SelectSpec()
            sel.num_columns, sel.num_rows = 1, 65537
            assert lib.pa_query_set_selection(h, ctypes.byref(sel)) == -4 and b"PA_MAX_SELECT_ROWS" in lib.pa_last_error()
            sel.num_rows = 5
            sel.columns[0] = g.column_ids["m"]
            assert lib.pa_query_set_selection(h, ctypes.byref(sel)) == 0
            assert lib.pa_query_bind_segment(h, 0, g.handle, (L.LeafParams * 1)(), None) == 0
            assert lib.pa_query_prepare(h) == -4 and b"multi-value" in lib.pa_last_error()
        finally:
            lib.pa_query_destroy(h)
    finally:
        g.close()
    ex = SelectionExecutor(parse_sql("SELECT a FROM t ORDER BY a LIMIT 5"), gsegs)
    try:
        ex.execute()
        assert L.lib().pa_query_fetch(ex.handle, None, 0, None, None, None) < 0
        assert b"pa_query_fetch_selection" in L.lib().pa_last_error()
        assert len(ex.fetch().rows) == 5
    finally:
        ex.close()
