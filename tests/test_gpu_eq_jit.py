"""The scan kernel compiled per query shape for one equality with rare survivors (csrc/eqs_jit.hip), against the oracle
and against the generic kernel (PA_QF_NO_JIT) of the same executor.

Tables are two segments of 3 * 2048 + 777 and 2 * 2048 + 1 docs. Tuning scan_grid = 1 leaves one workgroup of four
waves, so a wave walks several tiles, among them a ragged one, and crosses the segment switch; eq_jit = 1 takes the
kernel at every cardinality (on its own the planner wants a dictionary of at least 4096 values). The filter column f is
packed nb bits wide for every nb in 1..24; its dictionary holds 2^nb values where the literal is dictId 2^nb - 1 and
min(2^nb, 4096) values otherwise (the C-ABI takes the width per column). The literal's dictId sits only where it is
planted: docs 0, 31, 32, 2047, 2048, the last doc of each segment and, where the width has one, a doc whose field lies
across two 32-bit words. A second clause, a dictId range on column z, keeps some of the planted docs and drops others;
the query groups by g and aggregates COUNT, SUM over an INT dictionary and SUM over a LONG dictionary beyond int32.

Small dictionaries make the planner expect a dense result, for which it would choose LDS accumulators or the dense
kernel: those cases pin the direct kernel on global accumulators with PA_QF_NO_DENSE_GROUP | PA_QF_FORCE_GLOBAL, for
the kernel under test and the generic one alike.

Bars: pa_query_eq_jit as stated per case; group keys, COUNT, SUMs and numDocsScanned bit-equal to the oracle and to the
generic kernel; numEntriesScannedInFilter equal to the generic kernel's.
"""
import numpy as np
import pytest
import torch

import oracle
import width_tables as WT
from pinot_amd import _lib as L
from pinot_amd import parse_sql
from pinot_amd.engine import GpuQueryExecutor, GpuSegment
from pinot_amd.segment import pack_bits, segment_from_dict_ids
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

TILE = 2048
SEG_DOCS = (3 * TILE + 777, 2 * TILE + 1)
TUNE = {"scan_grid": 1, "eq_jit": 1}
PIN = L.PA_QF_NO_DENSE_GROUP | L.PA_QF_FORCE_GLOBAL
Z_KEEP = (3, 12)  # the second clause keeps z's dictIds 3..12 of 16
LANE_FULL = range(TILE + 5 * 32, TILE + 6 * 32)  # every doc of lane 5 of tile 1


def _straddler(nb, n):
    """The first doc past tile 1's first lane whose nb-bit field lies across two 32-bit words (None: no field does)."""
    for d in range(TILE + 33, min(n, TILE + 200)):
        if (d * nb) % 32 + nb > 32:
            return d
    return None


def _planted(nb, n):
    docs = [0, 31, 32, 2047, 2048, n - 1]
    s = _straddler(nb, n)
    return docs + ([s] if s is not None else [])


def _fdict(card, which=0):
    return 3 * np.arange(card, dtype=np.int64) + which


def _segment(nb, card, target, planted, seed, n, fdict=None, name="e"):
    """f holds `target` exactly at the docs `planted`, any other dictId elsewhere; z alternates inside / outside Z_KEEP
    over the planted docs; g, si, sl are seeded random."""
    rng = np.random.default_rng([seed, nb, n])
    fdict = _fdict(card) if fdict is None else fdict
    ids = rng.integers(0, card - 1, size=n, dtype=np.int64)
    ids[ids >= target] += 1  # uniform over the other dictIds
    near = [v for v in (target - 1, target + 1, target ^ 1, target ^ (1 << (nb - 1)), target ^ (1 << (nb // 2)))
            if 0 <= v < card and v != target]
    if near:
        where = rng.choice(n, size=n // 8, replace=False)
        ids[where] = rng.choice(near, size=len(where))
    z = rng.integers(0, 16, size=n, dtype=np.int64)
    for k, d in enumerate(planted):
        ids[d] = target
        z[d] = (Z_KEEP[0] + k % 10) if k % 3 != 2 else (0, 13, 15)[(k // 3) % 3]  # two kept, one dropped, ...
    g = rng.integers(0, 8, size=n, dtype=np.int64)
    si = rng.integers(0, 1000, size=n, dtype=np.int64)
    sl = rng.integers(0, 500, size=n, dtype=np.int64)
    specs = {
        "f": ("INT", fdict, np.zeros((n * nb + 7) // 8, dtype=np.uint8)),
        "z": ("INT", np.arange(16, dtype=np.int64) * 5, pack_bits(z.astype(np.uint32), 4)),
        "g": ("INT", np.arange(8, dtype=np.int64) * 10, pack_bits(g.astype(np.uint32), 3)),
        "si": ("INT", np.arange(1000, dtype=np.int64) * 7 - 3000, pack_bits(si.astype(np.uint32), 10)),
        "sl": ("LONG", np.arange(500, dtype=np.int64) * 1_000_003 - (1 << 40), pack_bits(sl.astype(np.uint32), 9)),
    }
    seg = segment_from_dict_ids("%s%d_%d_%d" % (name, nb, seed, n), n, specs)
    f = seg.column("f")
    f.num_bits = nb  # (wider than the dictionary needs where it is capped)
    f.fwd_bytes = pack_bits(ids.astype(np.uint32), nb)
    return seg


def _table(nb, card, target, seed, planted="std"):
    segs = []
    for k, n in enumerate(SEG_DOCS):
        if planted == "std":
            docs = _planted(nb, n)
        elif planted == "none":
            docs = []
        else:  # "lane": every doc of one lane of the first segment, nothing in the second
            docs = list(LANE_FULL) if k == 0 else []
        segs.append(_segment(nb, card, target, docs, seed + k, n))
    return segs


def _sql(value, where=None):
    where = where or "f IN (%d) AND z BETWEEN %d AND %d" % (value, 5 * Z_KEEP[0], 5 * Z_KEEP[1])
    return "SELECT g, COUNT(*), SUM(si), SUM(sl) FROM t WHERE %s GROUP BY g LIMIT 100" % where


def _flags(card):
    return PIN if card < 8192 else 0


def _run(sql, gsegs, flags=0, tuning=TUNE, execution_stats=True):
    q = parse_sql(sql)
    ex = GpuQueryExecutor(q, gsegs, flags=flags, tuning=tuning)
    try:
        plan = ex.stats()["plan"]
        jit = int(L.lib().pa_query_eq_jit(ex.handle))
        ex.execute()
        got = ex.fetch(execution_stats=execution_stats)
    finally:
        ex.close()
    return q, plan, jit, got


def _check(segs, sql, flags, want_groups=None):
    """The kernel under test runs, and gives the oracle's and the generic kernel's result and filter statistics."""
    gs = [GpuSegment(s) for s in segs]
    try:
        q, plan, jit, got = _run(sql, gs, flags)
        _, plan0, jit0, got0 = _run(sql, gs, flags | L.PA_QF_NO_JIT)
    finally:
        for g in gs:
            g.close()
    exp = oracle.run_query(q, segs)
    assert jit == 1 and jit0 == 0, (plan, plan0)
    assert plan["strategy"] == "global" and plan["variant"] == "global", plan
    assert_same(got, exp)
    assert_same(got0, exp)
    assert got.groups == got0.groups and got.num_docs_scanned == got0.num_docs_scanned
    assert got.num_entries_scanned_in_filter == got0.num_entries_scanned_in_filter
    assert got.num_entries_scanned_post_filter == got0.num_entries_scanned_post_filter
    if want_groups is not None:
        assert bool(exp.groups) == want_groups
    return exp


@pytest.mark.parametrize("nb", range(1, 25))
def test_every_width(nb):
    full, small = 1 << nb, min(1 << nb, 4096)
    cases = [(small, 0), (full, full - 1), (small, small // 2)]
    if nb == 1:
        cases = cases[:2]  # (a dictionary of two values has no middle one)
    for card, target in cases:
        segs = _table(nb, card, target, 10 * nb)
        exp = _check(segs, _sql(int(_fdict(card)[target])), _flags(card), want_groups=True)
        kept = sum(1 for n in SEG_DOCS for k in range(len(_planted(nb, n))) if k % 3 != 2)
        assert exp.num_docs_scanned == kept  # the planted docs the second clause keeps, and no other doc
    # no match at all; every doc of one lane
    segs = _table(nb, small, 0, 10 * nb + 3, planted="none")
    exp = _check(segs, _sql(int(_fdict(small)[0])), _flags(small), want_groups=False)
    assert exp.num_docs_scanned == 0
    segs = _table(nb, small, small - 1, 10 * nb + 5, planted="lane")
    exp = _check(segs, _sql(int(_fdict(small)[small - 1])), _flags(small), want_groups=True)
    assert exp.num_docs_scanned == sum(1 for k in range(32) if k % 3 != 2)


@pytest.fixture(scope="module")
def table17():
    segs = _table(17, 1 << 17, 70001, 170)
    gs = [GpuSegment(s) for s in segs]
    yield segs, gs, int(_fdict(1 << 17)[70001])
    for g in gs:
        g.close()


def _double(res):
    return {k: [2 * v for v in vals] for k, vals in res.groups.items()}


@pytest.mark.parametrize("external", [False, True], ids=["own_block", "external_block"])
def test_two_scans_after_one_reset_and_an_external_block(table17, external):
    """reset, scan, scan: doubled sums (COUNT and SUM only); with an accumulator block of the caller's the kernel's
    pointers follow pa_query_set_accumulator_buffer."""
    segs, gs, v = table17
    q = parse_sql(_sql(v))
    exp = oracle.run_query(q, segs)
    assert exp.groups
    ex = GpuQueryExecutor(q, gs, tuning=TUNE)
    keep = None
    try:
        assert int(L.lib().pa_query_eq_jit(ex.handle)) == 1
        assert int(L.lib().pa_query_leap_leaf(ex.handle)) >= 0  # the scan counts the filter statistics itself
        if external:
            n = int(L.lib().pa_query_accumulator_bytes(ex.handle))
            keep = torch.full((n + 512,), 0x5A, dtype=torch.uint8, device="cuda")  # (a dirty block: reset cleans it)
            base = keep.data_ptr() + (-keep.data_ptr()) % 256
            L.check(L.lib().pa_query_set_accumulator_buffer(ex.handle, base, n), "set_accumulator_buffer")
        ex.execute()
        assert_same(ex.fetch(execution_stats=False), exp)
        ex.reset()
        ex.scan()
        ex.scan()
        r = ex.fetch(execution_stats=False)
        assert r.num_docs_scanned == 2 * exp.num_docs_scanned
        assert r.groups == _double(exp)
        ex.execute()
        assert_same(ex.fetch(execution_stats=True), exp)
    finally:
        ex.close()


def test_segments_with_their_own_dictionaries_of_two_widths():
    """The value has another dictId, in a column of another width, in each segment: two width classes, the pattern and
    the tile's DMA change at the segment switch."""
    ta, tb = 2001, 1901
    da, db = _fdict(1 << 17), 300 + _fdict(1 << 13)
    assert da[ta] == db[tb]
    a = _segment(17, 1 << 17, ta, _planted(17, SEG_DOCS[0]), 31, SEG_DOCS[0], fdict=da)
    b = _segment(13, 1 << 13, tb, _planted(13, SEG_DOCS[1]), 32, SEG_DOCS[1], fdict=db)
    exp = _check([a, b], _sql(int(da[ta])), 0, want_groups=True)
    assert exp.num_docs_scanned > 0
    exp = _check([b, a], _sql(int(da[ta])), 0, want_groups=True)  # (and the narrow class first)


@pytest.mark.parametrize("card,want", [(1024, 0), (4096, 1)])
def test_auto_follows_the_dictionary(card, want):
    """Without the tuning the kernel runs behind a dictionary of 4096 values and not behind one of 1024."""
    nb = int(card - 1).bit_length()
    segs = _table(nb, card, card // 3, 77)
    gs = [GpuSegment(s) for s in segs]
    try:
        q, plan, jit, got = _run(_sql(int(_fdict(card)[card // 3])), gs, PIN, tuning={"scan_grid": 1})
        _, _, jit_off, _ = _run(_sql(int(_fdict(card)[card // 3])), gs, PIN, tuning={"scan_grid": 1, "eq_jit": 0})
    finally:
        for g in gs:
            g.close()
    assert jit == want and jit_off == 0, plan
    assert_same(got, oracle.run_query(q, segs))


def _refused(segs, sql, flags=0):
    gs = [GpuSegment(s) for s in segs]
    try:
        q, plan, jit, got = _run(sql, gs, flags, execution_stats=False)
    finally:
        for g in gs:
            g.close()
    assert jit == 0, (sql, plan)
    assert_same(got, oracle.run_query(q, segs))


def test_refusals():
    """Shapes outside the kernel's report pa_query_eq_jit == 0 under eq_jit = 1 and still give the oracle's result."""
    segs = _table(17, 1 << 17, 70001, 170)
    d = _fdict(1 << 17)
    v = int(d[70001])
    zr = "z BETWEEN %d AND %d" % (5 * Z_KEEP[0], 5 * Z_KEEP[1])
    for where in ("f <> %d AND %s" % (v, zr),                      # a negated equality
                  "f BETWEEN %d AND %d AND %s" % (v, v + 3, zr),   # a range of two dictIds
                  "f IN (%d) OR z IN (75)" % v,                    # an OR clause
                  "f IN (%d) AND z IN (15, 25, 60)" % v):          # a DICT_SET second clause
        _refused(segs, _sql(v, where))
    # 25 bits: beyond the prefilter's widths
    wide = [_segment(25, 1 << 20, 777, _planted(25, n), 250 + k, n) for k, n in enumerate(SEG_DOCS)]
    _refused(wide, _sql(int(_fdict(1 << 20)[777])))
    # a multi-value group-by column, and a raw group-by column (hashed key space)
    t = WT.build_table("m", 7)
    lo, hi = t.filter_bounds(0.0)
    _refused(t.segments, "SELECT m, COUNT(*) FROM t WHERE f IN (%d) GROUP BY m LIMIT 1000" % lo)
    _refused(t.segments, "SELECT rl, COUNT(*), SUM(v) FROM t WHERE f IN (%d) GROUP BY rl LIMIT 1000" % lo)
