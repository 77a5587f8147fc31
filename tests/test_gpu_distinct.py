"""Distinct queries on the GPU (engine.DistinctExecutor: the key-presence bitmap scan in its LDS and global variants and
the rank / order finish) against the restatement tests/distinct_ref.py under the completed comparator. Equality is
exact: rows in order, `present` = the number of distinct matching records, the statistics where they are defined and
None where not. The golden cases are the reference's own (tests/golden/sv_distinct.json); the synthetic shapes are the
ones at which the kernels can go wrong: ragged tiles, one-doc segments, per-segment dictionaries (remaps), bitmap words
shared or not within a 64-doc step, the first and last key of a key space, key spaces past 2^27, the largest key space
the LDS bitmap takes and the next one."""
import ctypes

import numpy as np
import pytest

import distinct_ref as R
from pinot_amd import _lib as L
from pinot_amd import parse_sql
from pinot_amd.segment import create_segment
from test_distinct import distinct_queries_table, golden

pytestmark = pytest.mark.gpu

LDS, GLOBAL = 129, 130            # pa_query_plan strategy codes (pa_device.h)
HI, LO = "\uffff", "\U00010000"  # String.compareTo: LO < HI (UTF-16 code units); by code point HI < LO
VARIANTS = [None, {"distinct_lds": 0}]


def _norm(rows):
    return [[repr(v) if isinstance(v, float) else v for v in r] for r in rows]


def plan_of(ex):
    vals = [ctypes.c_int32() for _ in range(7)]
    L.check(L.lib().pa_query_plan(ex.handle, *[ctypes.byref(v) for v in vals]), "plan")
    return dict(zip(("strategy", "steps", "dma_slots", "ring", "wg_per_cu", "grid", "lds_bytes"), [v.value for v in vals]))


def run_gpu(gsegs, query, tuning=None, force_scan=False, table_dicts=None):
    """(DistinctResult, plan or None) of one query over resident segments."""
    from pinot_amd.engine import DistinctExecutor
    ex = DistinctExecutor(query, gsegs, tuning=tuning, force_scan=force_scan, table_dicts=table_dicts)
    try:
        res = ex.run()
        return res, (plan_of(ex) if ex.handle is not None else None)
    finally:
        ex.close()


def count_stats(gsegs, query):
    """numEntriesScannedInFilter of the same WHERE, from the aggregation path (checked against the reference's golden
    statistics by the existing tests)."""
    from pinot_amd.engine import GpuQueryExecutor
    import dataclasses
    cq = dataclasses.replace(parse_sql("SELECT COUNT(*) FROM t"), filter=query.filter)
    ex = GpuQueryExecutor(cq, gsegs)
    try:
        return ex.run().num_entries_scanned_in_filter
    finally:
        ex.close()


def assert_same(got, ref, gsegs=None, query=None):
    assert list(got.columns) == list(ref.columns)
    assert _norm(got.rows) == _norm(ref.rows)
    assert got.present == ref.present
    assert got.num_total_docs == ref.total_docs
    if ref.stats_defined:
        assert got.num_docs_scanned == ref.matched
        assert got.num_entries_scanned_post_filter == ref.post
        if ref.fast_path:
            assert got.num_entries_scanned_in_filter == 0
        elif gsegs is not None:
            assert got.num_entries_scanned_in_filter == count_stats(gsegs, query)
    else:
        assert (got.num_docs_scanned, got.num_entries_scanned_in_filter, got.num_entries_scanned_post_filter) == \
            (None, None, None)


def check(gsegs, segs, sql, variants=VARIANTS, table_dicts=None, stats=False, expect=None):
    """One query in every variant against the restatement; returns the restatement's result."""
    q = parse_sql(sql)
    ref = R.completed_server(q, segs, force_scan=True)
    for tuning in variants:
        got, plan = run_gpu(gsegs, q, tuning=tuning, force_scan=True, table_dicts=table_dicts)
        assert plan is not None  # (force_scan: never the dictionary fast path)
        want = expect if (expect is not None and tuning is None) else (GLOBAL if tuning else LDS)
        assert plan["strategy"] == want, (sql, tuning, plan)
        assert_same(got, ref, gsegs if stats else None, q)
    return ref


def resident(segs):
    from pinot_amd.engine import GpuSegment
    ids = None
    out = []
    for s in segs:
        g = GpuSegment(s, device=0, column_ids=ids)
        ids = g.column_ids
        out.append(g)
    return out


def close_all(gsegs):
    for g in gsegs:
        g.close()


# ------------------------------------------------------------------ golden cases
@pytest.fixture(scope="module")
def golden_gpu(golden_segment):
    from pinot_amd.engine import GpuSegment
    g = GpuSegment(golden_segment, device=0)
    yield g
    g.close()


def test_golden_inner_segment(golden_gpu, golden_segment):
    """InnerSegmentDistinctSingleValueQueriesTest: 6582 records on the dictionary fast path and again through the scan;
    21968 records over K = 6582 x 21910 = 144,211,620 keys (> 2^27) on the global bitmap."""
    for case in golden()["inner_segment"]:
        q = parse_sql(case["sql"])
        vals = np.stack([R.SR.decoded(golden_segment, c) for c in q.select_columns], axis=1)
        uniq = np.unique(vals, axis=0)
        for force in (False, True):
            got, plan = run_gpu([golden_gpu], q, force_scan=force)
            assert got.columns == case["columns"] and got.column_types == case["types"]
            assert len(got.rows) == case["size"] and got.present == case["size"]
            assert sorted(tuple(r) for r in got.rows) == [tuple(r) for r in uniq.tolist()]
            ref = R.completed_server(q, [golden_segment], force_scan=force)
            assert_same(got, ref, [golden_gpu], q)
            if len(q.select_columns) == 1:
                assert (plan is None) == (not force)
                if not force:  # DictionaryBasedDistinctOperator.java:56-133: (n, 0, n, numDocs)
                    assert (got.num_docs_scanned, got.num_entries_scanned_in_filter,
                            got.num_entries_scanned_post_filter, got.num_total_docs) == (6582, 0, 6582, 30000)
            else:
                assert plan["strategy"] == GLOBAL
                assert (got.num_docs_scanned, got.num_entries_scanned_in_filter,
                        got.num_entries_scanned_post_filter) == (30000, 0, 60000)


def test_golden_distinct_queries():
    """The in-scope DistinctQueriesTest cases: one executor per segment, merged by reduce.merge_distinct."""
    from pinot_amd.reduce import merge_distinct
    spec = golden()
    segs = distinct_queries_table(spec)
    gsegs = resident(segs)
    try:
        for case in spec["distinct_queries"]["cases"]:
            q = parse_sql(case["sql"])
            for force in (False, True):
                parts = []
                for i in case["segments"]:
                    got, _ = run_gpu([gsegs[i]], q, force_scan=force)
                    assert_same(got, R.completed_server(q, [segs[i]], force_scan=force), [gsegs[i]], q)
                    parts.append(got)
                cols, rows = merge_distinct(parts, q)
                assert cols == list(q.select_columns)
                if "rows" in case:
                    assert rows == case["rows"], case["source"]
                else:
                    assert len(rows) == len(case["set"]), case["source"]
                    assert {r[0] if isinstance(r[0], str) else int(r[0]) for r in rows} == set(case["set"]), case["source"]
    finally:
        close_all(gsegs)


# ------------------------------------------------------------------ tile and segment edges
SIZES = (1, 63, 64, 2047, 2048, 2049, 4097)


@pytest.fixture(scope="module")
def ragged():
    """Segments of 1 .. 4097 docs, each with its own dictionaries (table-wide ids through remaps): three DISTINCT
    columns of table cardinalities 7 x 5 x 3 = 105 keys, a filter column f, a STRING column s."""
    rng = np.random.default_rng(7)
    segs = []
    for si, n in enumerate(SIZES):
        pool = np.array(["k%d" % i for i in range(1 + si)] + [HI, LO + "x"][: si % 3])
        data = {
            "a": (rng.integers(0, 1 + min(si, 6), n) * 3 + (si % 2) * 3).astype(np.int32) % 21,
            "b": (rng.integers(0, 1 + min(si, 4), n)).astype(np.int64) * 1000003,
            "c": (rng.integers(0, 3, n)).astype(np.float64) / 4 - 0.25,
            "f": ((np.arange(n) * 7 + si) % 50).astype(np.int32),
            "s": pool[rng.integers(0, len(pool), n)],
        }
        if si == 3:
            data["f"][:] = 49  # a segment none of whose docs match f < 40
        segs.append(create_segment("rag%d" % si, data, {"a": "INT", "b": "LONG", "c": "DOUBLE", "f": "INT", "s": "STRING"}))
    gsegs = resident(segs)
    yield segs, gsegs
    close_all(gsegs)


def test_key_space_of_105(ragged):
    segs, gsegs = ragged
    from pinot_amd.engine import DistinctExecutor
    ex = DistinctExecutor(parse_sql("SELECT DISTINCT a, b, c FROM t LIMIT 1000"), gsegs, force_scan=True)
    assert ex.num_keys == 105 and [len(d) for d in ex.global_dicts] == [7, 5, 3]
    ex.close()


@pytest.mark.parametrize("which", [[0], [1], [2], [3], [4], [5], [6], [0, 3, 5], list(range(7))])
def test_segment_edges(ragged, which):
    segs, gsegs = ragged
    ss, gg = [segs[i] for i in which], [gsegs[i] for i in which]
    check(gg, ss, "SELECT DISTINCT a, b, c FROM t LIMIT 1000", stats=True)
    check(gg, ss, "SELECT DISTINCT a, b, c FROM t WHERE f < 40 ORDER BY c DESC, a LIMIT 1000", stats=True)
    check(gg, ss, "SELECT DISTINCT b FROM t WHERE f >= 10 LIMIT 3")
    ref = check(gg, ss, "SELECT DISTINCT a, c FROM t WHERE f > 1000 LIMIT 10", stats=True)
    assert ref.rows == [] and ref.present == 0


def test_string_utf16_order(ragged):
    segs, gsegs = ragged
    for order in ("", "ORDER BY s DESC", "ORDER BY a DESC, s"):
        check(gsegs, segs, "SELECT DISTINCT s, a FROM t %s LIMIT 1000" % order)
    ref = check(gsegs, segs, "SELECT DISTINCT s FROM t WHERE f < 45 LIMIT 1000")
    col = [r[0] for r in ref.rows]
    assert col.index(LO + "x") < col.index(HI)  # by code point it would be the other way round


# ------------------------------------------------------------------ bitmap edges
def _one_column(values, card, name="k"):
    """A segment whose INT column k holds `values`, with the table-wide dictionary 0 .. card - 1."""
    seg = create_segment("edge", {name: np.asarray(values, dtype=np.int32),
                                  "f": (np.arange(len(values)) % 4).astype(np.int32)}, {name: "INT", "f": "INT"})
    return seg, {name: np.arange(card, dtype=np.int32)}


@pytest.mark.parametrize("name,values,card", [
    ("first_and_last_bits", [0, 31, 32, 32, 0, 31] * 40 + [32], 33),           # K = 33: keys 0, 31, 32 = K - 1
    ("k_not_multiple_of_32", list(range(0, 45, 2)) * 30 + [44], 45),
    ("one_key", [17] * 3000, 33),                                             # all 64 lanes on one bit
    ("64_words_per_step", [32 * (i % 64) for i in range(64 * 40)], 2048 + 5),  # 64 consecutive docs, 64 words
    ("two_keys_one_word", [(3 if i % 2 else 9) + 32 * ((i // 2) % 32) for i in range(4096 + 64)], 1024),
])
def test_bitmap_edges(name, values, card):
    seg, dicts = _one_column(values, card)
    gsegs = resident([seg])
    try:
        from pinot_amd.engine import DistinctExecutor
        ex = DistinctExecutor(parse_sql("SELECT DISTINCT k FROM t"), gsegs, force_scan=True, table_dicts=dicts)
        assert ex.num_keys == card
        ex.close()
        for sql in ("SELECT DISTINCT k FROM t LIMIT 100000", "SELECT DISTINCT k FROM t WHERE f > 0 ORDER BY k DESC LIMIT 100000",
                    "SELECT DISTINCT k FROM t WHERE f = 1 LIMIT 5"):
            ref = check(gsegs, [seg], sql, table_dicts=dicts, stats=True)
        assert ref.present == len(set(v for i, v in enumerate(values) if i % 4 == 1))
    finally:
        close_all(gsegs)


def test_largest_lds_key_space_and_the_next():
    """The largest K the planner gives the LDS bitmap, read from the plans it reports for this segment (a bisection over
    the table cardinality in whole bitmap words: prepare only, no scan), and K + 32, which must go global."""
    from pinot_amd.engine import DistinctExecutor
    n = 5000
    rng = np.random.default_rng(3)
    vals = rng.integers(0, 4000, n)
    seg, _ = _one_column(vals, 4000)
    gsegs = resident([seg])
    try:
        q = parse_sql("SELECT DISTINCT k FROM t LIMIT 100000")

        def strategy(k):
            ex = DistinctExecutor(q, gsegs, force_scan=True, table_dicts={"k": np.arange(k, dtype=np.int32)})
            try:
                return plan_of(ex)["strategy"]
            finally:
                ex.close()

        lo, hi = 4000 // 32 + 1, 160 * 1024 * 8 // 32 + 1  # words: LDS at lo, global at hi (past the LDS of a CU)
        assert strategy(32 * lo) == LDS and strategy(32 * hi) == GLOBAL
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if strategy(32 * mid) == LDS:
                lo = mid
            else:
                hi = mid
        k_max = 32 * lo
        assert 4000 < k_max < 160 * 1024 * 8
        # the bisection stands on the rule being monotonic in K: LDS up to k_max, global from there on
        for k in (32 * (4000 // 32 + 7), k_max // 2, k_max - 32):
            assert strategy(k) == LDS, k
        for k in (k_max + 64, 2 * k_max, 8 * k_max):
            assert strategy(k) == GLOBAL, k
        for k, want in ((k_max, LDS), (k_max + 32, GLOBAL)):
            # the values present include the last key of the space
            v = np.concatenate([vals, [k - 1, 0, k - 33]])
            s2, d2 = _one_column(v, k)
            g2 = resident([s2])
            try:
                ref = check(g2, [s2], "SELECT DISTINCT k FROM t LIMIT 100000", table_dicts=d2, expect=want)
                assert ref.rows[-1] == [k - 1]
                check(g2, [s2], "SELECT DISTINCT k FROM t ORDER BY k DESC LIMIT 3", table_dicts=d2, expect=want)
            finally:
                close_all(g2)
    finally:
        close_all(gsegs)


def test_large_direct_key_space():
    """16384 x 8193 = 134,234,112 keys (> 2^27, a 16 MiB bitmap), ~5000 docs including key 0 and key K - 1."""
    rng = np.random.default_rng(11)
    n = 5000
    x = rng.integers(0, 16384, n).astype(np.int32)
    y = rng.integers(0, 8193, n).astype(np.int32)
    x[:2], y[:2] = [0, 16383], [0, 8192]
    x[100:140], y[100:140] = x[60:100], y[60:100]  # duplicates
    seg = create_segment("big", {"x": x, "y": y}, {"x": "INT", "y": "INT"})
    dicts = {"x": np.arange(16384, dtype=np.int32), "y": np.arange(8193, dtype=np.int32)}
    gsegs = resident([seg])
    try:
        from pinot_amd.engine import DistinctExecutor
        ex = DistinctExecutor(parse_sql("SELECT DISTINCT x, y FROM t"), gsegs, table_dicts=dicts)
        assert ex.num_keys == 16384 * 8193 == 134234112 > 1 << 27
        ex.close()
        ref = check(gsegs, [seg], "SELECT DISTINCT x, y FROM t LIMIT 1000000", variants=[None], table_dicts=dicts,
                    expect=GLOBAL, stats=True)
        assert ref.rows[0] == [0, 0] and ref.rows[-1] == [16383, 8192] and ref.present == len(np.unique(np.stack([x, y], 1), axis=0))
        check(gsegs, [seg], "SELECT DISTINCT x, y FROM t ORDER BY y DESC LIMIT 10", variants=[None], table_dicts=dicts,
              expect=GLOBAL)
    finally:
        close_all(gsegs)


def test_fast_path_equals_scan_under_a_wider_table_dictionary():
    """A table-wide dictionary shared with other servers holds values no segment here has: the dictionary fast path
    answers from the bound segments' dictionaries, so it returns what the scan returns."""
    seg, dicts = _one_column([3, 40, 3, 17, 40, 5] * 50, 64)
    gsegs = resident([seg])
    try:
        for sql in ("SELECT DISTINCT k FROM t LIMIT 100", "SELECT DISTINCT k FROM t ORDER BY k DESC LIMIT 3"):
            q = parse_sql(sql)
            fast, plan = run_gpu(gsegs, q, table_dicts=dicts)
            scan, plan2 = run_gpu(gsegs, q, table_dicts=dicts, force_scan=True)
            assert plan is None and plan2 is not None
            assert fast.rows == scan.rows == R.completed_server(q, [seg]).rows
            assert fast.present == scan.present == 4
    finally:
        close_all(gsegs)


def test_fetch_refuses_a_scan_that_skipped_work():
    from pinot_amd.engine import DistinctExecutor
    seg, dicts = _one_column([1, 2, 3] * 100, 8)
    gsegs = resident([seg])
    try:
        ex = DistinctExecutor(parse_sql("SELECT DISTINCT k FROM t"), gsegs, force_scan=True, tuning={"debug_emit": 1})
        try:
            ex.execute()
            with pytest.raises(L.PinotAmdError, match="results invalid"):
                ex.fetch()
        finally:
            ex.close()
    finally:
        close_all(gsegs)


# ------------------------------------------------------------------ ordering and limits
def test_order_mixes_and_limits(ragged):
    segs, gsegs = ragged
    P = R.completed_server(parse_sql("SELECT DISTINCT a, b, c FROM t WHERE f < 40 LIMIT 100000"), segs, True).present
    assert P > 20
    for order in ("ORDER BY a, b, c", "ORDER BY a DESC, b, c DESC", "ORDER BY c DESC, b DESC, a DESC", "ORDER BY b DESC, a",
                  "ORDER BY b", "ORDER BY c DESC", ""):
        for limit in (1, P - 1, P, P + 1):
            ref = check(gsegs, segs, "SELECT DISTINCT a, b, c FROM t WHERE f < 40 %s LIMIT %d" % (order, limit), stats=True)
            assert len(ref.rows) == min(limit, P) and ref.present == P
    # ORDER BY a subset: the tie class at the cut is resolved by the completion (remaining columns ascending)
    ref = check(gsegs, segs, "SELECT DISTINCT a, b, c FROM t ORDER BY b DESC LIMIT 4")
    top = [r for r in R.completed_server(parse_sql("SELECT DISTINCT a, b, c FROM t LIMIT 1000"), segs, True).rows
           if r[1] == ref.rows[0][1]]
    assert ref.rows == sorted(top, key=lambda r: (r[0], r[2]))[:4]


def test_order_by_limit_65536_and_refusal():
    """300 x 300 values, all present (P = 90000 > 65536): ORDER BY with the largest limit; one more is refused."""
    from pinot_amd.engine import DistinctExecutor, UnsupportedQuery
    u, v = np.divmod(np.arange(90000), 300)
    rng = np.random.default_rng(2)
    p = rng.permutation(90000)
    seg = create_segment("sq", {"u": u[p].astype(np.int32), "v": v[p].astype(np.int32)}, {"u": "INT", "v": "INT"})
    gsegs = resident([seg])
    try:
        ref = check(gsegs, [seg], "SELECT DISTINCT u, v FROM t ORDER BY v DESC, u LIMIT 65536", stats=True)
        assert len(ref.rows) == 65536 and ref.present == 90000
        ref = check(gsegs, [seg], "SELECT DISTINCT u, v FROM t LIMIT 1000000", stats=True)
        assert len(ref.rows) == 90000
        with pytest.raises(UnsupportedQuery, match="PA_MAX_SELECT_ROWS"):
            DistinctExecutor(parse_sql("SELECT DISTINCT u, v FROM t ORDER BY v LIMIT 65537"), gsegs)
    finally:
        close_all(gsegs)


# ------------------------------------------------------------------ refusals
def test_refusals():
    from pinot_amd.engine import DistinctExecutor, UnsupportedQuery
    n = 100
    data = {"r": np.arange(n, dtype=np.int32), "d": (np.arange(n) % 7).astype(np.int32),
            "m": [np.array([i % 3, 5], dtype=np.int32) for i in range(n)],
            "x": (np.arange(n) % 5).astype(np.int32), "y": (np.arange(n) % 3).astype(np.int32)}
    schema = {"r": "INT", "d": "INT", "m": "INT", "x": "INT", "y": "INT"}
    seg = create_segment("ref", data, schema, no_dictionary_columns=("r",), multi_value_columns=("m",))
    gsegs = resident([seg])
    try:
        with pytest.raises(UnsupportedQuery, match="raw"):
            DistinctExecutor(parse_sql("SELECT DISTINCT r, d FROM t"), gsegs)
        with pytest.raises(UnsupportedQuery, match="multi-value"):
            DistinctExecutor(parse_sql("SELECT DISTINCT d, m FROM t"), gsegs)
        big = {c: np.arange(2048, dtype=np.int32) for c in ("d", "x", "y")}  # 2^33 keys from the cardinalities alone
        with pytest.raises(UnsupportedQuery, match="2\\^31"):
            DistinctExecutor(parse_sql("SELECT DISTINCT d, x, y FROM t"), gsegs, table_dicts=big)
        with pytest.raises(UnsupportedQuery, match="null handling"):
            DistinctExecutor(parse_sql("SELECT DISTINCT d FROM t OPTION(enableNullHandling=true)"), gsegs)
        ex = DistinctExecutor(parse_sql("SELECT DISTINCT d, x FROM t"), gsegs)
        try:
            ex.execute()
            rc = L.lib().pa_query_fetch(ex.handle, None, 0, None, None, None)
            assert rc == -1  # PA_EINVAL
            assert b"pa_query_fetch_distinct" in L.lib().pa_last_error()
            assert len(ex.fetch().rows) == 10  # (the distinct fetch still works after the refused call)
        finally:
            ex.close()
    finally:
        close_all(gsegs)


# ------------------------------------------------------------------ isolation
def test_other_families_unchanged_around_a_distinct_query(ragged):
    from pinot_amd.engine import GpuQueryExecutor, SelectionExecutor
    segs, gsegs = ragged

    def group():
        ex = GpuQueryExecutor(parse_sql("SELECT a, COUNT(*) FROM t WHERE f < 40 GROUP BY a TOP 1000"), gsegs)
        try:
            r = ex.run()
            return sorted(r.groups.items()), r.num_docs_scanned
        finally:
            ex.close()

    def select():
        ex = SelectionExecutor(parse_sql("SELECT a, b FROM t WHERE f < 40 ORDER BY b DESC, a LIMIT 20"), gsegs)
        try:
            r = ex.run()
            return r.rows, r.docs.tolist(), r.segments.tolist()
        finally:
            ex.close()

    before = group(), select()
    for tuning in VARIANTS:
        run_gpu(gsegs, parse_sql("SELECT DISTINCT a, b FROM t WHERE f < 40 LIMIT 100"), tuning=tuning)
    assert (group(), select()) == before
