"""FIRSTWITHTIME / LASTWITHTIME on the GPU (the row-by-time scan, STRAT_TROW_LDS = 135 and STRAT_TROW = 136, and the
finish kernel of pa_query_fetch_time_rows) against the plain-Python restatement (with_time_ref.py): equal (segment,
doc, value, time) for every group, exactly.

Table: three segments of 5,000, 2,049 and 1 docs (a ragged last tile, a doc just past a 2,048-doc wave tile, a
one-doc segment), every segment with its own dictionaries. Keys: g (12 values), h (about 3,000 values: most lanes of a
step own a key of their own), c (constant: one group hit by every lane, the wave pre-reduction). Times: td
(dictionary LONG, 7 distinct values: ties are the rule and the row part of the word decides), tr (raw LONG, distinct
values), tw (raw LONG holding Long.MIN_VALUE, Long.MAX_VALUE and values between: the wide form with no tuning)."""
import numpy as np
import pytest

import with_time_ref as W
from pinot_amd import _lib as L
from pinot_amd import parse_sql
from pinot_amd import query as Q
from pinot_amd import reduce as R
from pinot_amd import trim as TR
from pinot_amd.engine import (LONG_MAX, LONG_MIN, GpuQueryExecutor, GpuSegment, UnsupportedQuery, ValueTimePair,
                              java_cast, with_time_default)
from pinot_amd.segment import create_segment

pytestmark = pytest.mark.gpu

SCHEMA = {"g": "INT", "h": "INT", "c": "INT", "f": "INT", "vb": "INT", "vi": "INT", "vl": "LONG", "vf": "FLOAT",
          "vd": "DOUBLE", "vs": "STRING", "ri": "INT", "rl": "LONG", "rf": "FLOAT", "rd": "DOUBLE", "td": "LONG",
          "tr": "LONG", "tw": "LONG", "mv": "INT"}
RAW = ("ri", "rl", "rf", "rd", "tr", "tw")
SIZES = (5000, 2049, 1)
# the reference test's six declared types over dictionary columns, then the raw value columns
VALUES = [("vb", "BOOLEAN"), ("vi", "INT"), ("vl", "LONG"), ("vf", "FLOAT"), ("vd", "DOUBLE"), ("vs", "STRING"),
          ("ri", "INT"), ("rl", "LONG"), ("rf", "FLOAT"), ("rd", "DOUBLE")]


def synth(seed, n, base):
    rng = np.random.default_rng(seed)
    tw = rng.integers(-(1 << 62), 1 << 62, size=n).astype(np.int64) * 2
    tw[rng.integers(0, n, size=max(1, n // 50))] = LONG_MIN
    tw[rng.integers(0, n, size=max(1, n // 50))] = LONG_MAX
    data = {
        "g": (rng.integers(0, 12, size=n) * 5 + 3 + seed).astype(np.int32),
        "h": rng.integers(0, 3000, size=n).astype(np.int32),
        "c": np.full(n, 42, dtype=np.int32),
        "f": rng.integers(0, 10, size=n).astype(np.int32),
        "vb": rng.integers(0, 2, size=n).astype(np.int32),
        "vi": rng.integers(-500 - seed, 500, size=n).astype(np.int32),
        "vl": rng.integers(-300, 300 + seed, size=n).astype(np.int64) * 5_000_000_000,
        "vf": (rng.integers(0, 200 + seed, size=n) * 0.37 - 9).astype(np.float32),
        "vd": rng.integers(0, 400 + seed, size=n) * 1.1 - 50.0,
        "vs": np.array(["ab", "ac", "b", "cab", "abc%d" % seed, "zz"])[rng.integers(0, 6, size=n)],
        "ri": rng.integers(-(1 << 31), 1 << 31, size=n).astype(np.int32),
        "rl": rng.integers(-(1 << 62), 1 << 62, size=n).astype(np.int64),
        "rf": rng.standard_normal(n).astype(np.float32),
        "rd": rng.standard_normal(n) * 1e10,
        "td": (rng.integers(0, 7, size=n).astype(np.int64) - 3) * 1_000_000_007 + seed % 2,
        "tr": base + rng.permutation(n).astype(np.int64),   # distinct values over the table
        "tw": tw,
        "mv": [rng.integers(0, 5, size=k).astype(np.int32) for k in rng.integers(1, 3, size=n)],
    }
    return create_segment("wt%d" % seed, data, SCHEMA, no_dictionary_columns=RAW, multi_value_columns=("mv",)), data


@pytest.fixture(scope="module")
def table():
    parts = [synth(11 + i, n, 100_000 * i) for i, n in enumerate(SIZES)]
    gsegs = [GpuSegment(s) for s, _ in parts]
    yield [s for s, _ in parts], [d for _, d in parts], gsegs
    for g in gsegs:
        g.close()


WHERE = {"": lambda d: np.ones(len(d["f"]), dtype=bool), " WHERE f < 3": lambda d: d["f"] < 3,
         " WHERE f > 100": lambda d: d["f"] > 100}


_WINNERS = {}  # the restatement's winners of the module's table, computed once per (function, time column, key, filter, limit)


def expected(datas, q, where, limit=None, schema=SCHEMA):
    """Per aggregation of q (None for the others): {key: (segment, doc, ValueTimePair)} from the restatement."""
    out = []
    key = q.group_by[0] if q.group_by else None
    for a in q.aggregations:
        if a.function not in Q.WITH_TIME_FUNCTIONS:
            out.append(None)
            continue
        memo = (a.function, a.time_column, key, where, limit)
        if schema is not SCHEMA or memo not in _WINNERS:  # (only the shared table's winners are kept)
            segs = [(d[a.time_column], None if key is None else d[key].tolist(), WHERE[where](d)) for d in datas]
            win = W.table_winners(a.function, segs, limit)
            if schema is SCHEMA:
                _WINNERS[memo] = win
        else:
            win = _WINNERS[memo]
        out.append({k: (si, doc, ValueTimePair(java_cast(datas[si][a.column][doc], schema[a.column], a.data_type), t))
                    for k, (si, doc, t) in win.items()})
    return out


def check(sql, table, where="", flags=0, tuning=None, limit=None, executions=1, schema=SCHEMA):
    """Runs sql + where and compares every with-time aggregation with the restatement; returns (result, plan, section
    kinds) for further assertions."""
    _, datas, gsegs = table
    q = parse_sql(sql.replace("{W}", where))
    ex = GpuQueryExecutor(q, gsegs, flags=flags, tuning=tuning)
    try:
        for _ in range(executions):
            ex.execute()
            res = ex.fetch(execution_stats=False)
        plan = ex.stats()["plan"]
        exp = expected(datas, ex.query, where, limit, schema)
        for ai, (a, e) in enumerate(zip(ex.query.aggregations, exp)):
            if e is None:
                continue
            # the winning rows themselves (the fetch above read the same accumulator with its value columns)
            segs, docs, _ = ex.fetch_time_rows(ex.agg_map[ai], len(res.groups) if q.group_by else 1, [])
            if not q.group_by:
                got = {(): (int(segs[0]), int(docs[0]), res.row[ai])}
                if not e:
                    e = {(): (-1, -1, with_time_default(a.function, a.data_type))}
            else:
                assert len(res.groups) == len(segs)
                got = {k[0]: (int(s), int(d), vals[ai]) for (k, vals), s, d in zip(res.groups.items(), segs, docs)}
            assert got == e, (a.result_name, plan["variant"], [(k, got.get(k), e.get(k)) for k in e if got.get(k) != e[k]][:3])
        return res, plan, [kind for kind, _, _ in ex.sections()]
    finally:
        ex.close()


def select(function, time):
    return ", ".join("%s(%s, %s, '%s')" % (function, c, time, t) for c, t in VALUES)


# ------------------------------------------------------------------ the reference's test method on this table
@pytest.mark.parametrize("where", ["", " WHERE f < 3"])
@pytest.mark.parametrize("shape", ["", "g", "h", "c", "vb"])
@pytest.mark.parametrize("time", ["td", "tr", "tw"])
@pytest.mark.parametrize("function", ["LASTWITHTIME", "FIRSTWITHTIME"])
def test_all_declared_types(table, function, time, shape, where):
    sql = "SELECT %s%s FROM t{W}%s" % (shape + ", " if shape else "", select(function, time),
                                      " GROUP BY " + shape if shape else "")
    res, plan, _ = check(sql, table, where)
    assert plan["strategy"] == "time_rows"
    # one accumulator for all ten aggregations; tw takes the wide form with no tuning, the others the packed one
    assert list(plan["time_row_form"].values()) == [2 if time == "tw" else 1]


@pytest.mark.parametrize("group_by,columns", [("", 7), (" GROUP BY vi", 7), (" GROUP BY g", 8)])
def test_execution_statistics(table, group_by, columns):
    """(numDocsScanned, numEntriesScannedInFilter, numEntriesScannedPostFilter, totalDocs) = (docs, 0, 7 x docs, docs) for
    six value columns + the time column (LastWithTimeQueriesTest.java:225); a group-by column that is also a value
    column adds nothing (:329), another one adds one."""
    _, _, gsegs = table
    sel = ", ".join("LASTWITHTIME(%s, tr, '%s')" % (c, t) for c, t in VALUES[:6])
    ex = GpuQueryExecutor(parse_sql("SELECT %s FROM t%s LIMIT 100000" % (sel, group_by)), gsegs)
    try:
        ex.execute()
        res = ex.fetch()
        n = sum(SIZES)
        assert (res.num_docs_scanned, res.num_entries_scanned_in_filter, res.num_entries_scanned_post_filter,
                res.num_total_docs) == (n, 0, columns * n, n)
    finally:
        ex.close()


def test_filter_matching_nothing(table):
    for fn, t in (("LASTWITHTIME", LONG_MIN), ("FIRSTWITHTIME", LONG_MAX)):
        for time in ("td", "tw"):
            res, _, _ = check("SELECT %s FROM t{W}" % select(fn, time), table, " WHERE f > 100")
            assert [p.time for p in res.row] == [t] * len(VALUES)
            assert res.row[5] == ValueTimePair("", t) and res.row[1] == ValueTimePair(-(1 << 31), t)
            res, _, _ = check("SELECT g, %s FROM t{W} GROUP BY g" % select(fn, time), table, " WHERE f > 100")
            assert res.groups == {}


@pytest.mark.parametrize("wide", [-1, 1])
def test_docs_at_the_ends_of_the_time_domain_beat_the_default(wide):
    """Every doc at Long.MIN_VALUE (LAST) / Long.MAX_VALUE (FIRST): the greatest (segment, doc) wins, not the default
    pair, in the packed form (the time range is one value) and the wide one; a column holding both ends is wide."""
    schema = {"v": "LONG", "lo": "LONG", "hi": "LONG", "both": "LONG", "f": "INT"}
    parts = []
    for n in (70, 3):
        data = {"v": np.arange(n, dtype=np.int64) + 1000 * n, "lo": np.full(n, LONG_MIN), "hi": np.full(n, LONG_MAX),
                "both": np.where(np.arange(n) % 2 == 0, LONG_MIN, LONG_MAX), "f": np.zeros(n, dtype=np.int32)}
        parts.append((create_segment("e%d" % n, data, schema, no_dictionary_columns=("lo", "hi", "both")), data))
    gsegs = [GpuSegment(s) for s, _ in parts]
    small = ([s for s, _ in parts], [d for _, d in parts], gsegs)
    try:
        sql = ("SELECT LASTWITHTIME(v, lo, 'LONG'), FIRSTWITHTIME(v, hi, 'LONG'), LASTWITHTIME(v, both, 'LONG'), "
               "FIRSTWITHTIME(v, both, 'LONG') FROM t")
        res, plan, _ = check(sql, small, tuning=None if wide < 0 else {"time_rows_wide": wide}, schema=schema)
        assert list(plan["time_row_form"].values()) == ([1, 1, 2, 2] if wide < 0 else [2, 2, 2, 2])
        assert res.row == [ValueTimePair(3002, LONG_MIN), ValueTimePair(3002, LONG_MAX), ValueTimePair(3001, LONG_MAX),
                           ValueTimePair(3002, LONG_MIN)]
    finally:
        for g in gsegs:
            g.close()


def test_all_segments_empty():
    """Every segment given is empty: the executor plans over the placeholder of the agreed schema and scans nothing; an
    aggregation-only query returns the default pairs, a GROUP BY no groups."""
    from pinot_amd.segment import Segment
    schema = {"g": ("INT", True, True), "v": ("LONG", True, True), "s": ("STRING", True, True), "ts": ("LONG", False, True)}
    empty = [GpuSegment(Segment("e%d" % i, 0)) for i in range(2)]
    try:
        for group_by in ("", " GROUP BY g"):
            q = parse_sql("SELECT LASTWITHTIME(v, ts, 'LONG'), FIRSTWITHTIME(s, ts, 'STRING'), COUNT(*) FROM t" + group_by)
            ex = GpuQueryExecutor(q, empty, schema=schema)
            try:
                assert ex.placeholder is not None and ex.handle is not None
                ex.execute()
                res = ex.fetch(execution_stats=False)
                if group_by:
                    assert res.groups == {}
                else:
                    assert res.row == [ValueTimePair(LONG_MIN, LONG_MIN), ValueTimePair("", LONG_MAX), 0]
            finally:
                ex.close()
    finally:
        for g in empty:
            g.close()


# ------------------------------------------------------------------ plans: accumulators, tile sizes, forms
BOTH = ("SELECT {K}LASTWITHTIME(vl, {T}, 'LONG'), FIRSTWITHTIME(vs, {T}, 'STRING'), LASTWITHTIME(rd, {T}, 'DOUBLE'), "
        "COUNT(*), SUM(vi) FROM t{W}{G}")


@pytest.mark.parametrize("flags,variant", [(L.PA_QF_FORCE_LDS, "time_rows_lds"), (L.PA_QF_FORCE_GLOBAL, "time_rows_global"),
                                           (L.PA_QF_STEPS16, None), (L.PA_QF_STEPS32, None),
                                           (L.PA_QF_FORCE_LDS | L.PA_QF_STEPS16, "time_rows_lds"),
                                           (L.PA_QF_FORCE_GLOBAL | L.PA_QF_STEPS16, "time_rows_global")])
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("key", ["", "g", "h", "c"])
def test_accumulators_tiles_and_forms(table, key, wide, flags, variant):
    """Packed and forced wide form (tuning time_rows_wide) of the same queries under both accumulator variants and both
    tile sizes: identical results (both equal the restatement); in the wide form COUNT(*) and SUM next to the
    aggregations keep their single-pass values and numDocsScanned does not double."""
    _, datas, _ = table
    for time in ("tr", "td"):
        for where in ("", " WHERE f < 3"):
            sql = BOTH.replace("{K}", key + ", " if key else "").replace("{T}", time).replace(
                "{G}", " GROUP BY " + key + " LIMIT 100000" if key else "")
            res, plan, _ = check(sql, table, where, flags=flags, tuning={"time_rows_wide": wide})
            if variant:
                assert plan["variant"] == variant
            if flags & (L.PA_QF_STEPS16 | L.PA_QF_STEPS32):
                assert plan["steps"] == (16 if flags & L.PA_QF_STEPS16 else 32)
            # (a dictionary time column is always packed)
            assert set(plan["time_row_form"].values()) == {2 if wide and time == "tr" else 1}
            masks = [WHERE[where](d) for d in datas]
            assert res.num_docs_scanned == sum(int(m.sum()) for m in masks)
            if key:
                keys = np.concatenate([d[key][m] for d, m in zip(datas, masks)])
                vi = np.concatenate([d["vi"][m] for d, m in zip(datas, masks)]).astype(np.int64)
                for k, vals in res.groups.items():
                    assert vals[3] == int((keys == k[0]).sum()) and vals[4] == float(vi[keys == k[0]].sum())
            else:
                assert res.row[3] == sum(int(m.sum()) for m in masks)
                assert res.row[4] == float(sum(int(d["vi"][m].astype(np.int64).sum()) for d, m in zip(datas, masks)))


def test_sections_are_shared_per_time_column_and_function(table):
    one = "SELECT g, LASTWITHTIME(vl, tr, 'LONG'), LASTWITHTIME(vs, tr, 'STRING') FROM t GROUP BY g"
    _, plan, kinds = check(one, table)
    assert kinds.count(L.PA_ACC_TIME_ROW_U64) == 1 and kinds.count(L.PA_ACC_TIME_MAX_I64) == 0
    assert len(plan["time_row_form"]) == 1
    two = "SELECT g, LASTWITHTIME(vl, tr, 'LONG'), FIRSTWITHTIME(vl, tr, 'LONG') FROM t GROUP BY g"
    _, _, kinds = check(two, table)
    assert kinds.count(L.PA_ACC_TIME_ROW_U64) == 2
    cols = "SELECT g, LASTWITHTIME(vl, tr, 'LONG'), LASTWITHTIME(vl, td, 'LONG') FROM t GROUP BY g"
    _, _, kinds = check(cols, table)
    assert kinds.count(L.PA_ACC_TIME_ROW_U64) == 2
    _, plan, kinds = check(one, table, tuning={"time_rows_wide": 1})
    assert kinds.count(L.PA_ACC_TIME_ROW_U64) == 1 and kinds.count(L.PA_ACC_TIME_MAX_I64) == 1
    # a packed and a wide aggregation in one query: the packed word is complete after the first launch
    mixed = "SELECT g, LASTWITHTIME(vl, td, 'LONG'), FIRSTWITHTIME(vl, tw, 'LONG'), COUNT(*) FROM t GROUP BY g"
    _, plan, kinds = check(mixed, table)
    assert sorted(plan["time_row_form"].values()) == [1, 2] and kinds.count(L.PA_ACC_TIME_MAX_I64) == 1


@pytest.mark.parametrize("flags", [0, L.PA_QF_FORCE_LDS, L.PA_QF_FORCE_GLOBAL])
@pytest.mark.parametrize("wide", [0, 1])
def test_a_second_execute_resets_both_forms(table, wide, flags):
    for where in ("", " WHERE f < 3"):
        check("SELECT g, LASTWITHTIME(vl, tr, 'LONG'), FIRSTWITHTIME(vd, tr, 'DOUBLE'), COUNT(*) FROM t{W} GROUP BY g",
              table, where, flags=flags, tuning={"time_rows_wide": wide}, executions=2)
    check("SELECT LASTWITHTIME(vl, tr, 'LONG'), FIRSTWITHTIME(vd, tr, 'DOUBLE') FROM t", table, flags=flags,
          tuning={"time_rows_wide": wide}, executions=2)


@pytest.mark.parametrize("wide", [0, 1])
def test_num_groups_limit_walk(table, wide):
    """numGroupsLimit below the number of groups: every segment admits its first 50 keys (the prefix walk), and the
    winners are those of the admitted keys' docs, in both forms (the second launch sees the same admitted-key mask)."""
    sql = ("SELECT h, LASTWITHTIME(vl, tr, 'LONG'), FIRSTWITHTIME(vi, tr, 'INT'), COUNT(*) FROM t{W} GROUP BY h LIMIT 100000 "
           "OPTION(numGroupsLimit=50)")
    for where in ("", " WHERE f < 3"):
        res, plan, _ = check(sql, table, where, tuning={"time_rows_wide": wide}, limit=50)
        assert plan["limit_trimming"] == 2 and res.num_groups_limit_reached
        assert 50 <= len(res.groups) <= 101


def test_server_trim_falls_back_to_the_host(table):
    _, _, gsegs = table
    q = parse_sql("SELECT h, LASTWITHTIME(vl, tr, 'LONG') FROM t GROUP BY h ORDER BY lastwithtime(vl, tr, 'LONG') DESC "
                  "LIMIT 3 OPTION(minServerGroupTrimSize=10)")
    ex = GpuQueryExecutor(q, gsegs)
    try:
        ex.execute()
        trimmed = ex.fetch(execution_stats=False, server_trim=True)
        assert ex.last_trim["device"] is False and ex.last_trim["kept"] == 15 < ex.last_trim["groups"]
        full = ex.fetch(execution_stats=False)
        assert trimmed.groups == R.server_trim(full, ex.query).groups
        top = R.final_result_table(trimmed, ex.query)
        assert top == R.final_result_table(full, ex.query) and len(top) == 3
        # the library itself refuses the device trim of such a query, whatever the terms
        with pytest.raises(L.PinotAmdError) as e:
            ex.fetch_arrays(trim_spec=TR.build_spec([(L.PA_TRIM_COUNT, 0, 0, 0)], 5))
        assert e.value.code == L.PA_EUNSUPPORTED
    finally:
        ex.close()


# ------------------------------------------------------------------ limits
@pytest.mark.parametrize("sql,reason", [
    ("SELECT rl, LASTWITHTIME(vl, tr, 'LONG') FROM t GROUP BY rl", "hashed key space"),               # raw group-by column
    ("SELECT LASTWITHTIME(vl, tr, 'LONG') FROM t GROUP BY ADD(vi, 1)", "transform expressions"),      # expression key
    ("SELECT mv, LASTWITHTIME(vl, tr, 'LONG') FROM t GROUP BY mv", "multi-value"),                    # MV group-by column
    ("SELECT LASTWITHTIME(vl, tr, 'LONG'), SUMMV(mv) FROM t", "multi-value"),                         # MV aggregation column
    ("SELECT LASTWITHTIME(mv, tr, 'INT') FROM t", "multi-value value column"),
    ("SELECT LASTWITHTIME(vl, mv, 'LONG') FROM t", "multi-value time column"),
    ("SELECT LASTWITHTIME(ADD(vi, 1), tr, 'DOUBLE') FROM t", "over the transform expression"),
    ("SELECT FIRSTWITHTIME(vl, ADD(tr, 1), 'LONG') FROM t", "transform expression as its time column"),
    ("SELECT LASTWITHTIME(vl, vd, 'LONG') FROM t", "not INT or LONG"),
    ("SELECT LASTWITHTIME(vl, vs, 'LONG') FROM t", "not INT or LONG"),
    ("SELECT LASTWITHTIME(vl, tr, 'LONG') FILTER (WHERE f < 3) FROM t", "FILTER"),
    ("SELECT LASTWITHTIME(vl, tr, 'LONG'), SUM(vi) FILTER (WHERE f < 3) FROM t", "aggregation filters"),
    ("SELECT LASTWITHTIME(vl, tr, 'LONG') FROM t OPTION(enableNullHandling=true)", "null handling"),
    ("SELECT LASTWITHTIME(vl, tr, 'STRING') FROM t", "'STRING' over the LONG column"),
    ("SELECT LASTWITHTIME(vs, tr, 'LONG') FROM t", "'LONG' over the STRING column"),
    ("SELECT h, LASTWITHTIME(vl, tr, 'LONG') FROM t GROUP BY h OPTION(numGroupsLimit=50)", "first-position"),
])
def test_refusals(table, sql, reason):
    _, _, gsegs = table
    flags = L.PA_QF_NO_LIMIT_WALK if "numGroupsLimit" in sql else 0
    with pytest.raises(UnsupportedQuery, match=reason):
        GpuQueryExecutor(parse_sql(sql), gsegs, flags=flags).close()


def test_refusals_of_the_segments():
    """A time column that is dictionary-encoded in some segments only; a BYTES value column; a packed form forced on a
    range that does not fit."""
    n = 10
    data = {"v": np.arange(n, dtype=np.int64), "ts": np.arange(n, dtype=np.int64) * ((1 << 63) // n), "s": np.array(["a"] * n)}
    schema = {"v": "LONG", "ts": "LONG", "s": "STRING"}
    a = create_segment("a", data, schema)
    b = create_segment("b", data, schema, no_dictionary_columns=("ts",))
    ga, gb = GpuSegment(a), GpuSegment(b)
    try:
        with pytest.raises(UnsupportedQuery, match="dictionary-encoded in some segments only"):
            GpuQueryExecutor(parse_sql("SELECT LASTWITHTIME(v, ts, 'LONG') FROM t"), [ga, gb]).close()
        with pytest.raises(UnsupportedQuery, match="does not fit the packed form"):
            GpuQueryExecutor(parse_sql("SELECT LASTWITHTIME(v, ts, 'LONG') FROM t"), [gb], tuning={"time_rows_wide": 0}).close()
        a.columns["s"].data_type = "BYTES"
        with pytest.raises(UnsupportedQuery, match="BYTES value column"):
            GpuQueryExecutor(parse_sql("SELECT LASTWITHTIME(s, ts, 'STRING') FROM t"), [ga]).close()
    finally:
        ga.close()
        gb.close()
