"""Filtered aggregations on the GPU (the fused lane scan, STRAT_FILTERED_LDS = 131 and STRAT_FILTERED = 132) against
reference (a) of tests/filtered_ref.py: the composition of one oracle query per lane. Exact for counts, integer / long
sums, MIN / MAX, HLL registers, value sets, group keys, numDocsScanned, numEntriesScannedPostFilter and numTotalDocs;
DOUBLE sums within the relative 1e-9 tests/test_gpu_parity.py uses. Every case runs in both variants (tuning
filtered_lds 0 / 1, the strategy asserted through pa_query_plan) and at both tile sizes (PA_QF_STEPS16 / STEPS32).
The synthetic shapes are the smallest at which the kernel can go wrong: one-doc, 63 / 64 / 65-doc, one-tile +- 1 and
multi-tile segments, negated lanes over ragged tails, own and shared dictionaries, empty / full / whole-dictionary /
shared lanes, lane leaves on staged, unstaged and raw columns, hot and spread keys, wide sums, no GROUP BY, the filter
limit, the LDS boundary and every refusal."""
import ctypes
import socket

import numpy as np
import pytest

import filtered_ref as R
from pinot_amd import _lib as L
from pinot_amd import parse_sql
from pinot_amd.segment import create_segment
from test_filtered import CASES, DOUBLE_COLUMNS, GOLDEN_CASES, SCHEMA, make_segment, make_table

pytestmark = pytest.mark.gpu

LDS, GLOBAL = 131, 132  # pa_query_plan strategy codes (pa_device.h)
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
    ex = GpuQueryExecutor(q, gsegs, flags=flags, tuning=None if lds is None else {"filtered_lds": lds}, **kw)
    try:
        return ex.run(), plan_of(ex)
    finally:
        ex.close()


def check(sql, segs, gsegs, variants=VARIANTS, doubles=DOUBLE_COLUMNS):
    q = parse_sql(sql)
    ref = R.compose(q, segs)
    for lds, steps in variants:
        got, plan = run_gpu(q, gsegs, lds=lds, flags=steps)
        assert plan["strategy"] == (LDS if lds else GLOBAL), (sql, lds, plan)
        assert plan["steps"] == (32 if steps == L.PA_QF_STEPS32 else 16)
        R.assert_same(got, ref, double_sum_columns=doubles)
    return ref


# ------------------------------------------------------------------ golden segment
@pytest.fixture(scope="module")
def golden_gpu(golden_segment):
    g = resident([golden_segment])
    yield g
    close_all(g)


@pytest.mark.parametrize("name", sorted(GOLDEN_CASES))
def test_golden(golden_gpu, golden_segment, name):
    ref = check(GOLDEN_CASES[name], [golden_segment], golden_gpu)
    assert ref.num_docs_scanned > 0


# ------------------------------------------------------------------ synthetic shapes
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2049, 5000])
def test_segment_sizes(n):
    """Every query shape over one segment of n docs with its own dictionaries next to two that share theirs."""
    segs = make_table(n)
    gsegs = resident(segs)
    try:
        for name in sorted(CASES):
            check(CASES[name], segs, gsegs)
    finally:
        close_all(gsegs)


def _keyed_segment(name, keys, seed):
    rng = np.random.default_rng(seed)
    n = len(keys)
    data = {c: np.zeros(n, dtype=np.int32) for c in SCHEMA}
    data["g"] = np.asarray(keys, dtype=np.int32)
    data["f1"] = rng.integers(0, 10, size=n).astype(np.int32)
    data["f2"] = rng.integers(0, 8, size=n).astype(np.int32)
    data["x"] = rng.integers(-7, 43, size=n).astype(np.int32)
    # multiples of 2^40 (beyond int32: the exact long pair): every partial sum is a double, and the totals pass 2^53
    data["y"] = (rng.integers(1 << 10, 1 << 12, size=n).astype(np.int64)) << 40
    data["d"] = (rng.integers(0, 40, size=n) * 0.37 - 3.0).astype(np.float64)
    data["s"] = np.array(["a"] * n, dtype=object)
    data["r"] = rng.integers(0, 100, size=n).astype(np.int32)
    return create_segment(name, data, SCHEMA, no_dictionary_columns=["r"])


KEYED_SQL = ("SELECT g, SUM(x) FILTER (WHERE f1 < 6), SUM(y) FILTER (WHERE f1 < 6), MIN(d) FILTER (WHERE f2 <> 3), "
             "MAX(x) FILTER (WHERE f2 <> 3), SUM(y), COUNT(*) FROM t GROUP BY g LIMIT 100000")


def test_hot_key_and_wide_sums():
    """Every doc in one group in every lane (the grouped pre-reduction); LONG sums whose totals pass 2^53."""
    segs = [_keyed_segment("hot", np.full(6000, 42), 1), _keyed_segment("hot2", np.full(2100, 42), 2)]
    gsegs = resident(segs)
    try:
        ref = check(KEYED_SQL, segs, gsegs)
        assert len(ref.groups) == 1 and ref.groups[(42,)][1] > 2.0 ** 53 and ref.groups[(42,)][4] > 2.0 ** 53
    finally:
        close_all(gsegs)


def test_spread_keys():
    """64 distinct keys in every 64-doc step (the ungrouped path: every lane updates its own key)."""
    segs = [_keyed_segment("spread", np.arange(4200) % 1024, 3)]
    gsegs = resident(segs)
    try:
        ref = check(KEYED_SQL, segs, gsegs)
        assert len(ref.groups) == 1024
    finally:
        close_all(gsegs)


def test_filter_limit():
    from pinot_amd.engine import UnsupportedQuery
    segs = [make_segment("lim", 300, 9, full=True)]
    gsegs = resident(segs)
    try:
        lanes = ", ".join("SUM(x) FILTER (WHERE f1 = %d)" % i for i in range(8))
        check("SELECT g, %s, COUNT(*) FROM t GROUP BY g LIMIT 1000" % lanes, segs, gsegs)
        with pytest.raises(UnsupportedQuery, match="more than 8 aggregation filters"):
            run_gpu(parse_sql("SELECT g, %s, SUM(x) FILTER (WHERE f1 = 8) FROM t GROUP BY g" % lanes), gsegs)
        wide = ", ".join("COUNT(*) FILTER (WHERE f1 = %d OR f2 = %d OR r = %d)" % (i, i, i) for i in range(6))
        with pytest.raises(UnsupportedQuery, match="more than 16 leaves"):
            run_gpu(parse_sql("SELECT g, %s FROM t GROUP BY g" % wide), gsegs)
    finally:
        close_all(gsegs)


def test_lds_boundary():
    """The largest key space the LDS variant takes by the planner's own rule, and the next one: found by asking
    pa_query_plan over growing K (the table-wide dictionary of the group-by column sets K)."""
    from pinot_amd.engine import GpuQueryExecutor
    segs = [_keyed_segment("k", np.arange(3000) % 700, 4)]
    gsegs = resident(segs)
    sql = "SELECT g, SUM(x) FILTER (WHERE f1 < 6), COUNT(*) FROM t GROUP BY g LIMIT 100000"
    q = parse_sql(sql)

    def strategy(k):
        ex = GpuQueryExecutor(q, gsegs, table_dicts={"g": np.arange(k, dtype=np.int32)})
        try:
            return plan_of(ex)["strategy"]
        finally:
            ex.close()
    try:
        lo, hi = 700, 1 << 20
        assert strategy(lo) == LDS and strategy(hi) == GLOBAL
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if strategy(mid) == LDS else (lo, mid)
        ref = R.compose(q, segs)
        for k, want in ((lo, LDS), (hi, GLOBAL)):
            got, plan = run_gpu(q, gsegs, table_dicts={"g": np.arange(k, dtype=np.int32)})
            assert plan["strategy"] == want
            R.assert_same(got, ref)
    finally:
        close_all(gsegs)


def test_refusals():
    from pinot_amd.engine import UnsupportedQuery
    rng = np.random.default_rng(5)
    n = 400
    schema = {"k": "INT", "big1": "INT", "big2": "INT", "raw": "INT", "mv": "INT", "m": "INT"}
    data = {"k": rng.integers(0, 300, n).astype(np.int32), "big1": np.arange(n, dtype=np.int32),
            "big2": rng.permutation(n).astype(np.int32), "raw": rng.integers(0, 9, n).astype(np.int32),
            "mv": [rng.integers(0, 5, size=1 + i % 3).astype(np.int32) for i in range(n)],
            "m": rng.integers(0, 50, n).astype(np.int32)}
    seg = create_segment("refuse", data, schema, no_dictionary_columns=["raw"], multi_value_columns=["mv"])
    gsegs = resident([seg])
    cases = [
        ("SELECT raw, SUM(m) FILTER (WHERE k < 5) FROM t GROUP BY raw", "hashed key space"),
        ("SELECT k, SUMMV(mv) FILTER (WHERE k < 5) FROM t GROUP BY k", "multi-value"),
        ("SELECT mv, SUM(m) FILTER (WHERE k < 5) FROM t GROUP BY mv", "multi-value"),
        ("SELECT k, SUM(m) FILTER (WHERE mv = 3) FROM t GROUP BY k", "multi-value column in an aggregation filter"),
        ("SELECT k, PERCENTILE50(m) FILTER (WHERE k < 5) FROM t GROUP BY k", "VALUE_HISTOGRAM"),
        ("SELECT k, PERCENTILE50(m), SUM(m) FILTER (WHERE k < 5) FROM t GROUP BY k", "VALUE_HISTOGRAM"),
        ("SELECT k, SUM(m) FILTER (WHERE k < 5) FROM t GROUP BY k OPTION(numGroupsLimit=10)", "numGroupsLimit"),
    ]
    try:
        for sql, message in cases:
            with pytest.raises(UnsupportedQuery, match=message):
                run_gpu(parse_sql(sql), gsegs)
        # a multi-value leaf of the main filter is allowed
        q = parse_sql("SELECT k, SUM(m) FILTER (WHERE k < 150), COUNT(*) FROM t WHERE mv = 3 GROUP BY k LIMIT 1000")
        got, _ = run_gpu(q, gsegs)
        import oracle
        import dataclasses
        plain = oracle.run_query(dataclasses.replace(q, aggregations=[q.aggregations[1]], aliases=[None]), [seg])
        assert {k: v[1] for k, v in got.groups.items()} == {k: v[0] for k, v in plain.groups.items()}
    finally:
        close_all(gsegs)


def test_constant_filters():
    """FILTER (WHERE TRUE) runs in the main lane, FILTER (WHERE FALSE) is a lane without docs."""
    segs = make_table(300)
    gsegs = resident(segs)
    try:
        q = parse_sql("SELECT g, SUM(x) FILTER (WHERE TRUE), MIN(x) FILTER (WHERE FALSE), COUNT(*) FILTER (WHERE f1 = 1 AND "
                      "FALSE), SUM(x) FILTER (WHERE f1 = 2 OR FALSE), COUNT(*) FROM t WHERE f2 < 7 GROUP BY g LIMIT 1000")
        got, _ = run_gpu(q, gsegs)
        plain, _ = run_gpu(parse_sql("SELECT g, SUM(x), SUM(x) FILTER (WHERE f1 = 2), COUNT(*) FROM t WHERE f2 < 7 GROUP BY "
                                     "g LIMIT 1000"), gsegs)
        assert set(got.groups) == set(plain.groups)
        for k, v in plain.groups.items():
            assert got.groups[k] == [v[0], float("inf"), 0, v[1], v[2]]
    finally:
        close_all(gsegs)


@pytest.mark.parametrize("sql", [
    "SELECT SUM(x) FILTER (WHERE TRUE) FROM t",                      # one lane, no lane on the device
    "SELECT SUM(x) FILTER (WHERE TRUE), COUNT(*) FROM t",            # match-all WHERE: TRUE stays a lane of its own
    "SELECT g, SUM(x) FILTER (WHERE TRUE), MIN(x) FILTER (WHERE FALSE) FROM t WHERE f2 < 7 GROUP BY g LIMIT 1000",
    "SELECT g, SUM(y) FILTER (WHERE TRUE), COUNT(*) FROM t WHERE f2 < 7 GROUP BY g LIMIT 1000",  # TRUE joins the main lane
    "SELECT MAX(x) FILTER (WHERE FALSE) FROM t WHERE f1 = 3",
])
def test_constant_only_filters_statistics(sql):
    """FILTER clauses that all fold to constants leave no lane on the device; the results and numDocsScanned /
    numEntriesScannedPostFilter still follow the lanes (every segment of the table, and its first alone)."""
    segs = make_table(300)
    gsegs = resident(segs)
    try:
        q = parse_sql(sql)
        for k in (len(segs), 1):
            ref = R.compose(q, segs[:k])
            got, _ = run_gpu(q, gsegs[:k])
            assert ref.num_total_docs > 0
            R.assert_same(got, ref, double_sum_columns=DOUBLE_COLUMNS)
    finally:
        close_all(gsegs)


def test_set_agg_filters_refusals_c_abi():
    """pa_query_set_agg_filters' PA_EINVAL paths through ctypes (the engine builds no such spec): counts out of range, a
    filter no aggregation uses, a bad program length, a malformed program, a filter index out of range, and a call
    after the first bind or after prepare."""
    from pinot_amd.engine import GpuQueryExecutor
    lib = L.lib()

    def spec_of(ex):
        fs = L.AggFilterSpec()
        fs.num_filters = len(ex.dev_filters)
        for j, fops in enumerate(ex.dev_filter_ops):
            fs.num_ops[j] = len(fops)
            for i, op in enumerate(fops):
                fs.ops[j][i] = op
        for i in range(L.PA_MAX_AGGS):
            fs.agg_filter[i] = ex.pa_agg_filter[i] if i < len(ex.pa_agg_filter) else -1
        return fs

    def attempt(handle, fs):
        rc = lib.pa_query_set_agg_filters(handle, None if fs is None else ctypes.byref(fs))
        return rc, lib.pa_last_error().decode(errors="replace") if rc else ""

    after_bind = []

    class AfterBind(GpuQueryExecutor):
        def _before_prepare(self):
            super()._before_prepare()
            after_bind.append(attempt(self.handle, spec_of(self)))

    segs = make_table(300)
    gsegs = resident(segs)
    q = parse_sql("SELECT g, SUM(x) FILTER (WHERE f1 < 5), COUNT(*) FROM t GROUP BY g LIMIT 1000")
    ex = AfterBind(q, gsegs)
    fresh = None
    try:
        assert len(after_bind) == 1 and after_bind[0][0] == L.PA_EINVAL and "before binding segments" in after_bind[0][1]
        rc, msg = attempt(ex.handle, spec_of(ex))
        assert rc == L.PA_EINVAL and "already prepared" in msg
        filtered = [i for i, f in enumerate(ex.pa_agg_filter) if f == 0]
        assert len(ex.dev_filters) == 1 and filtered
        fresh = L.check_ptr(lib.pa_query_create(ctypes.byref(ex.spec), len(ex.segs)), "pa_query_create")

        def bad(message, **change):
            fs = spec_of(ex)
            for name, value in change.items():
                if name == "num_filters":
                    fs.num_filters = value
                elif name == "num_ops":
                    fs.num_ops[0] = value
                elif name == "agg_filter":
                    fs.agg_filter[filtered[0]] = value
                elif name == "second":  # a copy of filter 0 as filter 1, which no aggregation uses
                    fs.num_filters = 2
                    fs.num_ops[1] = fs.num_ops[0]
                    for i in range(fs.num_ops[0]):
                        fs.ops[1][i] = fs.ops[0][i]
                elif name == "program":
                    fs.num_ops[0] = len(value)
                    for i, op in enumerate(value):
                        fs.ops[0][i] = op
            rc, msg = attempt(fresh, fs)
            assert rc == L.PA_EINVAL and message in msg, (change, rc, msg)

        assert attempt(fresh, None)[0] == L.PA_EINVAL
        bad("filters", num_filters=0)
        bad("filters", num_filters=L.PA_MAX_AGG_FILTERS + 1)
        bad("no aggregation uses", second=True)
        bad("bad program length", num_ops=0)
        bad("bad program length", num_ops=L.PA_MAX_OPS + 1)
        bad("index out of range", agg_filter=1)
        bad("index out of range", agg_filter=-2)
        bad("malformed filter program", program=[L.PA_OP_AND])  # an operator without operands
        bad("missing leaf", program=[L.PA_OP_LEAF | (200 << 8)])
        assert attempt(fresh, spec_of(ex)) == (L.PA_OK, "")  # (the same handle takes the well-formed spec)
    finally:
        if fresh:
            lib.pa_query_destroy(fresh)
        ex.close()
        close_all(gsegs)


# ------------------------------------------------------------------ multi-GPU
MULTI_SQL = ("SELECT g, h, SUM(x) FILTER (WHERE f1 < 5), AVG(y) FILTER (WHERE f2 = 1), MIN(d) FILTER (WHERE f2 = 1), "
             "DISTINCTCOUNTHLL(x) FILTER (WHERE f1 < 5), MAX(x), COUNT(*) FROM t WHERE f2 < 7 GROUP BY g, h LIMIT 1000")


def _table_dicts(q, segs):
    return {c: np.unique(np.concatenate([s.column(c).dictionary for s in segs])) for c in q.group_by}


def test_two_executors_sections_added_by_hand(rccl_world1):
    """Two executors over disjoint halves of the segments, their sections reduced on the device with torch by the
    section table's operations, equal one executor over all of them."""
    import torch
    import torch.distributed as dist
    from pinot_amd.engine import GpuQueryExecutor
    from pinot_amd.parallel import SECTION_OP, DistributedAccumulators
    segs = make_table(700) + [make_segment("own_b", 900, 77)]
    q = parse_sql(MULTI_SQL)
    td = _table_dicts(q, segs)
    gsegs = resident(segs)
    exs = [GpuQueryExecutor(q, gsegs[:2], table_dicts=td), GpuQueryExecutor(q, gsegs[2:], table_dicts=td)]
    try:
        accs = [DistributedAccumulators(e, torch.device("cuda", 0)) for e in exs]
        for e in exs:
            e.execute()
        torch.cuda.synchronize()
        assert L.PA_ACC_LANE_COUNT_U64 in [k for k, _, _ in exs[0].sections()]
        for (k0, t0), (k1, t1) in zip(accs[0].views, accs[1].views):
            assert k0 == k1 and t0.shape == t1.shape
            op = SECTION_OP[k0]
            if op == dist.ReduceOp.SUM:
                t0.add_(t1)
            elif op == dist.ReduceOp.MIN:
                torch.minimum(t0, t1, out=t0)
            else:
                torch.maximum(t0, t1, out=t0)
        torch.cuda.synchronize()
        got = exs[0].fetch(execution_stats=False)
        one, _ = run_gpu(q, gsegs, table_dicts=td)
        R.assert_same(got, one, double_sum_columns=DOUBLE_COLUMNS, stats=False, totals=False)
        R.assert_same(one, R.compose(q, segs), double_sum_columns=DOUBLE_COLUMNS)
    finally:
        for e in exs:
            e.close()
        close_all(gsegs)


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture(scope="module")
def rccl_world1():
    import torch
    import torch.distributed as dist
    dist.init_process_group("nccl", rank=0, world_size=1, init_method="tcp://127.0.0.1:%d" % _port(),
                            device_id=torch.device("cuda", 0))
    yield
    dist.destroy_process_group()


def test_distributed_accumulators_world1(rccl_world1):
    import torch
    from pinot_amd.engine import GpuQueryExecutor
    from pinot_amd.parallel import DistributedAccumulators
    segs = make_table(700)
    q = parse_sql(MULTI_SQL)
    gsegs = resident(segs)
    ex = GpuQueryExecutor(q, gsegs, table_dicts=_table_dicts(q, segs))
    try:
        acc = DistributedAccumulators(ex, torch.device("cuda", 0))
        ex.execute()
        torch.cuda.synchronize()
        with pytest.raises(L.PinotAmdError, match="no merged execution statistics"):
            acc.reduce(dst=0, execution_stats=True)
        acc.reduce(dst=0, execution_stats=False)
        got = ex.fetch(execution_stats=False)
        R.assert_same(got, R.compose(q, segs), double_sum_columns=DOUBLE_COLUMNS, stats=False)
        with pytest.raises(L.PinotAmdError, match="execution"):
            ex.fetch(execution_stats=True)
    finally:
        ex.close()
        close_all(gsegs)
