"""Transform expressions on the GPU (the expression scan, STRAT_EXPR_LDS = 133 and STRAT_EXPR = 134) against
tests/transform_ref.py: the same query over the materialised raw column through the unmodified oracle. Every case runs
in both variants (tuning expr_lds 1 / 0; a GROUP BY with an expression item has a hashed key space, which only 134 runs)
and at both tile sizes (PA_QF_STEPS32 / PA_QF_STEPS16), the strategy asserted through pa_query_plan.
numEntriesScannedPostFilter is checked against numDocsScanned x the distinct columns read.
The hashed table's overflow report is reached with the tuning hash_slots_cap (the planner's own table holds twice the
docs)."""
import ctypes
import math

import numpy as np
import pytest

import transform_ref as R
from pinot_amd import _lib as L
from pinot_amd import parse_sql
from pinot_amd import query as Q
from pinot_amd import transform as T
from pinot_amd.segment import create_segment
from test_transform import CASES, GOLDEN, RAW, SCHEMA, golden_segment, make_segment, make_table

pytestmark = pytest.mark.gpu

LDS, GLOBAL = 133, 134  # pa_query_plan strategy codes (pa_device.h)
VARIANTS = [(lds, steps) for lds in (1, 0) for steps in (L.PA_QF_STEPS32, L.PA_QF_STEPS16)]


def plan_of(ex):
    vals = [ctypes.c_int32() for _ in range(7)]
    L.check(L.lib().pa_query_plan(ex.handle, *[ctypes.byref(v) for v in vals]), "plan")
    return dict(zip(("strategy", "steps", "dma_slots", "ring", "wg_per_cu", "grid", "lds_bytes"), [v.value for v in vals]))


def resident(segs):
    from pinot_amd.engine import GpuSegment
    ids, out = None, []
    for s in segs:
        g = GpuSegment(s, device=0, column_ids=ids)
        ids = g.column_ids
        out.append(g)
    return out


def close_all(gsegs):
    for g in gsegs:
        g.close()


def run_gpu(q, gsegs, lds=None, flags=0, **kw):
    from pinot_amd.engine import GpuQueryExecutor
    ex = GpuQueryExecutor(q, gsegs, flags=flags, tuning=None if lds is None else {"expr_lds": lds}, **kw)
    try:
        return ex.run(), plan_of(ex)
    finally:
        ex.close()


def check(sql, segs, gsegs, exact=True, variants=VARIANTS, ref=None):
    q = parse_sql(sql)
    assert not exact or R.double_sums_exact(q, segs), sql  # (exact comparison only where every partial sum is a double)
    ref, mags = ref if ref is not None else R.reference(q, segs)
    hashed = any(isinstance(g, Q.Expr) for g in q.group_by)
    for lds, steps in variants:
        got, plan = run_gpu(q, gsegs, lds=lds, flags=steps)
        assert plan["strategy"] == (LDS if lds and not hashed else GLOBAL), (sql, lds, plan)
        assert plan["steps"] == (32 if steps == L.PA_QF_STEPS32 else 16)
        R.assert_same(got, ref, q, mags, exact=exact)
        assert got.num_entries_scanned_post_filter == R.post_filter_entries(q, ref.num_docs_scanned), sql
    return ref


# ------------------------------------------------------------------ the reference's golden results
@pytest.fixture(scope="module")
def golden4():
    segs = [golden_segment(i) for i in range(4)]
    g = resident(segs)
    yield segs, g
    close_all(g)


@pytest.mark.parametrize("i", range(7))
def test_golden(golden4, i):
    """TransformQueriesTest.java:164-263: the inner-segment (sum, count) pairs on one segment, the inter-segment averages
    over four copies of it."""
    segs, gsegs = golden4
    inner, inter = GOLDEN["inner_segment"][i], GOLDEN["inter_segment"][i]
    q = parse_sql(inner["query"])
    for lds, steps in VARIANTS:
        got, plan = run_gpu(q, gsegs[:1], lds=lds, flags=steps)
        assert plan["strategy"] == (LDS if lds else GLOBAL)
        assert (got.row[0].sum, got.row[0].count) == (inner["sum"], inner["count"])
        got, _ = run_gpu(parse_sql(inter["query"]), gsegs, lds=lds, flags=steps)
        assert got.row[0].count == 40 and got.row[0].sum / got.row[0].count == inter["avg"]
    check(inner["query"], segs, gsegs)


def test_golden_refused(golden4):
    from pinot_amd.engine import UnsupportedQuery
    _, gsegs = golden4
    for case in GOLDEN["failing"] + GOLDEN["datetrunc_refused"]:
        with pytest.raises(UnsupportedQuery):
            run_gpu(parse_sql(case["query"]), gsegs)


# ------------------------------------------------------------------ synthetic shapes
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2049, 5000])
def test_segment_sizes(n):
    """Every query shape over one segment of n docs with its own dictionaries next to two that share theirs."""
    segs = make_table(n)
    gsegs = resident(segs)
    try:
        for name in sorted(CASES):
            sql, exact = CASES[name]
            check(sql, segs, gsegs, exact=exact)
    finally:
        close_all(gsegs)


def _keyed(name, keys, seed):
    rng = np.random.default_rng(seed)
    n = len(keys)
    data = {c: np.zeros(n, dtype=np.int32) for c in SCHEMA}
    data["g"] = np.asarray(keys, dtype=np.int32)
    data["di"] = rng.integers(-7, 43, n)
    data["dl"] = rng.integers(1 << 10, 1 << 12, n).astype(np.int64) << 40
    data["ri"] = rng.integers(0, 100, n)
    data["rl"] = np.asarray(keys, dtype=np.int64) * 1000 + rng.integers(0, 1000, n)
    data["rd"] = rng.integers(0, 40, n) * 0.5
    data["dd"] = data["df"] = np.ones(n)
    data["s"] = np.array(["a"] * n, dtype=object)
    return create_segment(name, data, SCHEMA, no_dictionary_columns=RAW)


KEYED = [
    "SELECT g, SUM(ADD(di, ri)), SUM(timeConvert(dl, 'SECONDS', 'MILLISECONDS')), MIN(SUB(rd, di)), MAX(MULT(ri, rd)), "
    "SUM(dl), COUNT(*) FROM t GROUP BY g LIMIT 100000",
    "SELECT COUNT(*), SUM(ADD(di, ri)), MAX(dl) FROM t GROUP BY timeConvert(rl, 'MILLISECONDS', 'SECONDS') LIMIT 100000",
    "SELECT COUNT(*), SUM(MULT(ri, rd)) FROM t GROUP BY g, FLOOR(DIV(rl, 1000)) LIMIT 100000",
]


def test_hot_key():
    """Every doc in one group (the grouped pre-reduction across the wave); LONG sums whose totals pass 2^53."""
    segs = [_keyed("hot", np.full(6000, 42), 1), _keyed("hot2", np.full(2100, 42), 2)]
    gsegs = resident(segs)
    try:
        for sql in KEYED:
            ref = check(sql, segs, gsegs)
            assert len(ref.groups) == 1
        assert R.reference(parse_sql(KEYED[0]), segs)[0].groups[(42,)][1] > 2.0 ** 53
    finally:
        close_all(gsegs)


def test_spread_keys():
    """64 distinct keys in every 64-doc step (every lane updates its own key)."""
    segs = [_keyed("spread", np.arange(4200) % 1024, 3)]
    gsegs = resident(segs)
    try:
        for sql in KEYED:
            ref = check(sql, segs, gsegs)
            assert len(ref.groups) == 1024
    finally:
        close_all(gsegs)


def _bits_reference(q, segs, key_exprs):
    """Groups by the expressions' value bits in numpy (the oracle's map merges -0.0 with 0.0 and splits NaNs)."""
    groups = {}
    for s in segs:
        cols = [R.expr_values(e, s) for e in key_exprs]
        for i in range(s.num_docs):
            k = R.key_bits(tuple(c[i].item() for c in cols))
            groups[k] = groups.get(k, 0) + 1
    return groups


def test_special_double_keys():
    """Expression keys NaN (one group, whatever the NaN's bits), +-inf, -0.0 and 0.0 (two groups)."""
    n = 700
    rng = np.random.default_rng(5)
    data = {c: np.zeros(n, dtype=np.int32) for c in SCHEMA}
    data["rd"] = rng.choice(np.array([0.0, -0.0, 1.0, -1.0, math.inf, -math.inf, math.nan, 2.5]), n)
    data["dd"] = rng.choice(np.array([0.0, 1.0, -2.0, math.inf]), n)
    data["di"] = rng.integers(0, 3, n)
    data["s"] = np.array(["a"] * n, dtype=object)
    segs = [create_segment("special", data, SCHEMA, no_dictionary_columns=RAW)]
    gsegs = resident(segs)
    try:
        # MULT keeps the zero's sign; DIV makes inf and NaN (0/0, inf/inf); SUB makes NaN (inf - inf)
        for text in ("MULT(rd, dd)", "DIV(rd, dd)", "SUB(rd, dd)"):
            q = parse_sql("SELECT COUNT(*), SUM(di) FROM t GROUP BY %s LIMIT 1000" % text)
            want = _bits_reference(q, segs, q.group_by)
            for lds, steps in VARIANTS:
                got, plan = run_gpu(q, gsegs, lds=lds, flags=steps)
                assert plan["strategy"] == GLOBAL
                have = {R.key_bits(k): v[0] for k, v in got.groups.items()}
                assert len(have) == len(got.groups) and have == want, text
                assert all(isinstance(k[0], float) for k in got.groups)
            nan = ("d", 0x7ff8000000000000)
            assert (nan,) in want
        zeros = _bits_reference(None, segs, [parse_sql("SELECT SUM(MULT(rd, dd)) FROM t").aggregations[0].column])
        assert (("d", 0),) in zeros and (("d", 1 << 63),) in zeros
    finally:
        close_all(gsegs)


def test_saturated_long_keys():
    """LONG keys at TIMECONVERT's saturation values (Long.MAX_VALUE is the hashed table's empty marker: its own slot)."""
    n = 300
    data = {c: np.zeros(n, dtype=np.int32) for c in SCHEMA}
    data["rl"] = np.resize(np.array([2**62, -2**62, 106751, 106752, -106752, 0, 5, -5], dtype=np.int64), n)
    data["rd"] = np.resize(np.array([1e30, -1e30, math.nan, 3.0]), n)
    data["s"] = np.array(["a"] * n, dtype=object)
    segs = [create_segment("sat", data, SCHEMA, no_dictionary_columns=RAW)]
    gsegs = resident(segs)
    try:
        ref = check("SELECT COUNT(*), MAX(timeConvert(rl, 'DAYS', 'NANOSECONDS')), MIN(timeConvert(rl, 'DAYS', 'NANOSECONDS')) "
                    "FROM t GROUP BY timeConvert(rl, 'DAYS', 'NANOSECONDS') LIMIT 1000", segs, gsegs)
        assert (2**63 - 1,) in ref.groups and (-2**63,) in ref.groups
        ref = check("SELECT COUNT(*) FROM t GROUP BY timeConvert(rd, 'SECONDS', 'MILLISECONDS'), "
                    "timeConvert(rl, 'DAYS', 'HOURS') LIMIT 1000", segs, gsegs)
        assert {k[0] for k in ref.groups} == {2**63 - 1, -2**63, 0, 3000}
    finally:
        close_all(gsegs)


def test_shared_operand_and_plain_aggregations():
    """The same operand column in several expressions is one gather and one projected column; plain aggregations and
    group-by columns next to expression ones."""
    segs = make_table(900)
    gsegs = resident(segs)
    try:
        sql = ("SELECT g, SUM(ADD(di, ri)), SUM(SUB(di, ri)), MAX(MULT(di, di)), SUM(di), MIN(ri), MAX(dd), COUNT(*) FROM t "
               "GROUP BY g LIMIT 1000")
        ref = check(sql, segs, gsegs)
        assert R.post_filter_entries(parse_sql(sql), ref.num_docs_scanned) == 4 * ref.num_docs_scanned  # g, di, ri, dd
    finally:
        close_all(gsegs)


def test_limits():
    from pinot_amd.engine import UnsupportedQuery
    segs = make_table(200)
    gsegs = resident(segs)
    try:
        eight = ", ".join("SUM(ADD(di, %d))" % i for i in range(8))
        check("SELECT %s FROM t" % eight, segs, gsegs)
        with pytest.raises(UnsupportedQuery, match="more than 8 transform expressions"):
            run_gpu(parse_sql("SELECT %s, SUM(ADD(di, 8)) FROM t" % eight), gsegs)
        check("SELECT SUM(ADD(%s)) FROM t" % ", ".join(["di"] * 8), segs, gsegs)  # 16 operations
        with pytest.raises(UnsupportedQuery, match="more than 16 operations"):
            run_gpu(parse_sql("SELECT SUM(ADD(%s)) FROM t" % ", ".join(["di"] * 9)), gsegs)
        check("SELECT SUM(ADD(g, h, f, di, dl, df, dd, ri)) FROM t", segs, gsegs)  # 8 operand columns
        with pytest.raises(UnsupportedQuery, match="more than 8 distinct columns"):
            run_gpu(parse_sql("SELECT SUM(ADD(g, h, f, di, dl, df, dd, ri, rl)) FROM t"), gsegs)
    finally:
        close_all(gsegs)


def test_library_refusals():
    """What the C-ABI refuses: a malformed program (PA_EINVAL), numGroupsLimit trimming (PA_EUNSUPPORTED)."""
    from pinot_amd.engine import GpuQueryExecutor, UnsupportedQuery
    segs = make_table(400)
    gsegs = resident(segs)
    try:
        with pytest.raises(UnsupportedQuery, match="numGroupsLimit"):
            run_gpu(parse_sql("SELECT COUNT(*) FROM t GROUP BY ADD(rl, ri) OPTION(numGroupsLimit=50)"), gsegs)
        ex = GpuQueryExecutor(parse_sql("SELECT SUM(ADD(di, ri)) FROM t"), gsegs)
        try:
            good = T.fill_spec(ex.programs, [ex.gsegs[0].column_ids[c] for c in ex.expr_columns], [0], [])
            lib = L.lib()

            def rc_of(mutate):
                spec = L.ExprSpec.from_buffer_copy(good)
                mutate(spec)
                h = L.check_ptr(lib.pa_query_create(ctypes.byref(ex.spec), len(ex.segs)), "pa_query_create")
                try:
                    return lib.pa_query_set_expressions(h, ctypes.byref(spec))
                finally:
                    lib.pa_query_destroy(h)
            assert rc_of(lambda s: None) == L.PA_OK
            bad = {
                "programs": lambda s: setattr(s, "num_exprs", L.PA_MAX_EXPRS + 1),
                "columns": lambda s: setattr(s, "num_columns", L.PA_MAX_EXPR_COLUMNS + 1),
                "operations": lambda s: setattr(s.exprs[0], "num_ops", L.PA_MAX_EXPR_OPS + 1),
                "unused expression": lambda s: s.agg_expr.__setitem__(0, -1),
                "expression index": lambda s: s.agg_expr.__setitem__(0, 3),
                "register before definition": lambda s: setattr(s.exprs[0].ops[1], "b", 5),
                "register range": lambda s: setattr(s.exprs[0].ops[0], "dst", L.PA_MAX_EXPR_REGS),
                "operand type": lambda s: setattr(s.exprs[0].ops[0], "b", L.PA_EXPR_LONG),
                "result type": lambda s: setattr(s.exprs[0], "result_type", L.PA_EXPR_LONG),
                "column index": lambda s: setattr(s.exprs[0].ops[0], "a", 7),
                "opcode": lambda s: setattr(s.exprs[0].ops[1], "op", 99),
            }
            for what, mutate in bad.items():
                assert rc_of(mutate) == L.PA_EINVAL, what
            # after a bind (and after prepare) the call is refused: a bind reads the columns it replaces
            assert lib.pa_query_set_expressions(ex.handle, ctypes.byref(good)) == L.PA_EINVAL
        finally:
            ex.close()
        # TCONV's immediate: a valid program (LOAD_COL long, TCONV_MUL 1000), then its immediate made 0, negative, a
        # register
        ex = GpuQueryExecutor(parse_sql("SELECT SUM(timeConvert(dl, 'SECONDS', 'MILLISECONDS')) FROM t"), gsegs)
        try:
            assert [op[0] for op in ex.programs[0].ops] == [L.PA_EXPR_LOAD_COL, L.PA_EXPR_TCONV_MUL]
            good = T.fill_spec(ex.programs, [ex.gsegs[0].column_ids[c] for c in ex.expr_columns], [0], [])
            assert rc_of(lambda s: None) == L.PA_OK
            assert rc_of(lambda s: setattr(s.exprs[0].ops[1], "b_imm", 0)) == L.PA_EINVAL
            assert rc_of(lambda s: setattr(s.exprs[0].ops[1], "b_imm", -1000)) == L.PA_EINVAL
            assert rc_of(lambda s: setattr(s.exprs[0].ops[1], "b_kind", L.PA_EXPR_ARG_REG)) == L.PA_EINVAL
            assert rc_of(lambda s: setattr(s.exprs[0].ops[1], "b_kind", L.PA_EXPR_ARG_F64)) == L.PA_EINVAL
        finally:
            ex.close()
    finally:
        close_all(gsegs)


def test_lds_boundary():
    """STRAT_LDS's rule: the block (u32 counts + one DOUBLE sum: 12 bytes a key) takes at most 64 KiB. 60 x 91 = 5460
    keys fit (65520 bytes), 43 x 127 = 5461 do not (65552)."""
    n = 6000
    for (c1, c2), want in (((60, 91), LDS), ((43, 127), GLOBAL)):
        data = {c: np.zeros(n, dtype=np.int32) for c in SCHEMA}
        data["g"], data["h"] = np.arange(n) % c1, np.arange(n) % c2
        data["di"], data["ri"] = np.arange(n) % 17, np.arange(n) % 5
        data["s"] = np.array(["a"] * n, dtype=object)
        segs = [create_segment("b%d" % c1, data, SCHEMA, no_dictionary_columns=RAW)]
        gsegs = resident(segs)
        try:
            q = parse_sql("SELECT g, h, SUM(ADD(di, ri)) FROM t GROUP BY g, h LIMIT 100000")
            got, plan = run_gpu(q, gsegs)
            assert plan["strategy"] == want, (c1, c2, plan)
            ref, mags = R.reference(q, segs)
            R.assert_same(got, ref, q, mags)
        finally:
            close_all(gsegs)


def test_default_num_groups_limit_refuses_large_segments():
    """At default options (numGroupsLimit 100000) an expression key over a raw operand can take as many values as the
    segment has docs, so a segment of 100000 docs or more is refused (trimming is not built for expression keys); a
    smaller one runs, and so does the large one once its key is bounded by its operands' dictionaries."""
    from pinot_amd.engine import UnsupportedQuery
    big = make_segment("big", 100000, 11)
    gsegs = resident([big])
    try:
        with pytest.raises(UnsupportedQuery, match="numGroupsLimit"):
            run_gpu(parse_sql("SELECT COUNT(*) FROM t GROUP BY timeConvert(ts, 'MILLISECONDS', 'DAYS')"), gsegs)
        check("SELECT COUNT(*) FROM t GROUP BY ADD(di, MULT(g, 100)) LIMIT 1000", [big], gsegs, variants=VARIANTS[:1])
    finally:
        close_all(gsegs)
    small = make_segment("small", 99999, 12)
    gsegs = resident([small])
    try:
        check("SELECT COUNT(*) FROM t GROUP BY timeConvert(ts, 'MILLISECONDS', 'DAYS') LIMIT 1000", [small], gsegs,
              variants=VARIANTS[:1])
    finally:
        close_all(gsegs)


def test_hashed_table_overflow():
    """More distinct keys than the table has slots (tuning hash_slots_cap = 1024, about 5000 keys): docs whose key finds
    no slot are dropped in the scan (key_slot) and counted, and fetch fails with the report a raw key gets, for one-word
    and two-word keys."""
    from pinot_amd.engine import GpuQueryExecutor
    n = 5000
    data = {c: np.zeros(n, dtype=np.int32) for c in SCHEMA}
    data["rl"] = np.arange(n, dtype=np.int64) * 7
    data["g"] = np.arange(n) % 3
    data["s"] = np.array(["a"] * n, dtype=object)
    segs = [create_segment("many", data, SCHEMA, no_dictionary_columns=RAW)]
    gsegs = resident(segs)
    try:
        for sql in ("SELECT COUNT(*), SUM(ADD(di, ri)) FROM t GROUP BY ADD(rl, 1) LIMIT 100000",                # one word
                    "SELECT COUNT(*) FROM t GROUP BY g, timeConvert(rl, 'SECONDS', 'MILLISECONDS') LIMIT 100000",  # two
                    "SELECT COUNT(*) FROM t GROUP BY rl LIMIT 100000",                                        # a raw key
                    "SELECT COUNT(*) FROM t GROUP BY g, rl LIMIT 100000"):
            q = parse_sql(sql)
            for steps in (L.PA_QF_STEPS32, L.PA_QF_STEPS16):
                ex = GpuQueryExecutor(q, gsegs, flags=steps, tuning={"hash_slots_cap": 1024})
                try:
                    assert ex.hashed and ex.num_keys == 1025 and ex.key_words == (2 if " g, " in sql else 1)
                    ex.execute()
                    with pytest.raises(L.PinotAmdError, match="group-key table overflow"):
                        ex.fetch()
                finally:
                    ex.close()
            # the same query with the table the planner sizes runs
            got, _ = run_gpu(q, gsegs)
            assert len(got.groups) == n
    finally:
        close_all(gsegs)
