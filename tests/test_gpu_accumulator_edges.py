"""Accumulators at their limits: integer sums far past 2^53 (rounded once, ties to even), negative and cancelling
totals, a hot key at the packed dense fields' capacity, integer MIN / MAX at the int64 / int32 extremes, doubles at the
ends of the order encoding — through every accumulation path, each test asserting from the plan that its path ran.

The reference is neither the oracle nor the engine: the oracle adds doubles in docId order and is itself inexact past
2^53. Here the expected SUM of an integer column is float(exact) of the exact Python-int total (CPython's float(int)
rounds to nearest, ties to even: the double of the exact sum), expected MIN / MAX are float(value), and integer results
are compared with ==, no tolerance anywhere. Double MIN / MAX are compared bit for bit; a double SUM holding one
infinity must be that infinity, holding both must be NaN; a finite double SUM lies within n * 2^-52 * sum(|x|) of
math.fsum — the first-order bound (n - 1) u sum|x| (u = 2^-53) of recursive summation in ANY order of n terms, with a
factor of two to spare for the higher-order terms; derived, not measured.

Designed groups (TARGETS): every group holds a handful of LONG values that add up exactly to a chosen total — ties in
both directions at 2^53 and above, the carry of an all-ones significand into the next binade, a tie with one sticky bit,
+/-2^63, +/-2^64 and neighbours, 0 / 1 / -1 from parts near +/-2^62 (cancellation), a low-32 partial sum that crosses
2^32 under a negative high part, INT64_MIN and INT64_MAX alone and together. Widths up to 2^95 are covered on the host
by tests/test_round_host.py.

Out of scope: NaN inputs, and +0.0 next to -0.0 in one group. The reference implementation disagrees with itself on
both (MinAggregationFunction.aggregate uses Math.min, aggregateGroupBySV uses value < current), so matching it depends
on docId order: a design decision, not a test.
"""
import math
import struct

import numpy as np
import pytest

from pinot_amd import _lib as L
from pinot_amd import parse_sql
from pinot_amd.engine import GpuQueryExecutor, GpuSegment
from pinot_amd.segment import create_segment

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
DBL_MAX = float(np.finfo(np.float64).max)
FLT_MAX = float(np.finfo(np.float32).max)
FLT_SUB = float(np.float32(1e-45))  # the smallest float subnormal, 2^-149
INT_TYPES = ("INT", "LONG")


# ------------------------------------------------------------------ the reference
def exact_group_sums(values, inverse, ngroups):
    """Exact per-group sums of int64 `values` as Python ints, by the split the engine uses: the low 32 bits (unsigned)
    and the high 32 bits (signed) are summed apart in 64-bit words (no overflow below 2^31 values), then recombined in
    arbitrary precision."""
    v = np.asarray(values, dtype=np.int64)
    assert len(v) < (1 << 31)
    lo = np.zeros(ngroups, dtype=np.uint64)
    hi = np.zeros(ngroups, dtype=np.int64)
    np.add.at(lo, inverse, (v & np.int64(0xffffffff)).astype(np.uint64))
    np.add.at(hi, inverse, v >> np.int64(32))
    return [int(h) * (1 << 32) + int(l) for h, l in zip(hi.tolist(), lo.tolist())]


class DoubleSum:
    """The expected SUM of doubles: fsum and the bound of any summation order, or the infinity / NaN it must be."""

    def __init__(self, xs):
        xs = [float(x) for x in xs]
        pinf, ninf = any(x == math.inf for x in xs), any(x == -math.inf for x in xs)
        self.special = math.nan if pinf and ninf else math.inf if pinf else -math.inf if ninf else None
        fin = [x for x in xs if math.isfinite(x)]
        self.value = math.fsum(fin)
        # n * 2^-52 * sum|x| (module docstring); sum|x| itself in extended precision
        try:
            self.bound = len(fin) * 2.0 ** -52 * math.fsum(abs(x) for x in fin)
        except OverflowError:  # (DBL_MAX and -DBL_MAX in one sum: the bound itself is past the doubles)
            self.bound = math.inf

    def matches(self, got):
        if self.special is not None:
            return math.isnan(got) if math.isnan(self.special) else got == self.special
        return abs(got - self.value) <= self.bound


def reference(cols, types, mask, group_by, aggs, times=1):
    """{group key tuple: [expected value per aggregation]} over the docs of `mask` ({(): [...]} without GROUP BY, also
    when nothing matches). cols: {column: numpy array over all bound segments}; aggs: [(function, column)]. COUNT is an
    int, an integer SUM float(exact Python int), integer MIN / MAX float(value), double MIN / MAX the value itself, a
    double SUM a DoubleSum. times: every doc counts that many times (the same segments bound several times)."""
    idx = np.flatnonzero(mask) if mask is not None else np.arange(len(next(iter(cols.values()))))
    if group_by:
        keys = np.stack([np.asarray(cols[c])[idx].astype(np.int64) for c in group_by], axis=1)
        uniq, inverse = np.unique(keys, axis=0, return_inverse=True)
        inverse = inverse.reshape(-1)
        names = [tuple(r) for r in uniq.tolist()]
    else:
        inverse = np.zeros(len(idx), dtype=np.int64)
        names = [()]
    ng = len(names)
    counts = np.bincount(inverse, minlength=ng).tolist()
    order_counts = counts
    counts = [c * times for c in counts]
    order = np.argsort(inverse, kind="stable")
    bounds = np.concatenate([[0], np.cumsum(order_counts)]).astype(np.int64)
    out = [[] for _ in range(ng)]
    for fn, col in aggs:
        if fn == "COUNT":
            for g in range(ng):
                out[g].append(counts[g])
            continue
        v = np.asarray(cols[col])[idx]
        if types[col] in INT_TYPES:
            v = v.astype(np.int64)
            if fn == "SUM":
                res = [float(s * times) for s in exact_group_sums(v, inverse, ng)]
            else:
                ident = I64_MAX if fn == "MIN" else I64_MIN
                acc = np.full(ng, ident, dtype=np.int64)
                (np.minimum if fn == "MIN" else np.maximum).at(acc, inverse, v)
                res = [float(x) if c else (math.inf if fn == "MIN" else -math.inf) for x, c in zip(acc.tolist(), counts)]
        else:
            sv = v.astype(np.float64)[order]
            res = []
            for g in range(ng):
                xs = sv[bounds[g]:bounds[g + 1]].tolist()
                if fn == "SUM":
                    res.append(DoubleSum(xs * times))
                elif not xs:
                    res.append(math.inf if fn == "MIN" else -math.inf)
                else:
                    res.append(min(xs) if fn == "MIN" else max(xs))
        for g in range(ng):
            out[g].append(res[g])
    return {k: out[g] for g, k in enumerate(names) if group_by == [] or counts[g]}


def bits(x):
    return struct.pack("<d", float(x))


def assert_matches(got, want, aggs, types, group_by):
    """got: the engine's IntermediateResult; want: reference()."""
    if group_by:
        assert set(got.groups) == set(want), sorted(set(got.groups) ^ set(want))[:8]
        rows = [(k, got.groups[k], want[k]) for k in want]
    else:
        rows = [((), got.row, want[()])]
    for k, g, w in rows:
        assert len(g) == len(w) == len(aggs)
        for (fn, col), a, b in zip(aggs, g, w):
            if isinstance(b, DoubleSum):
                assert b.matches(float(a)), (k, fn, col, a, b.special, b.value, b.bound)
            elif fn == "COUNT":
                assert int(a) == b and float(a) == float(b), (k, fn, a, b)
            elif types[col] in INT_TYPES:
                assert float(a) == b, (k, fn, col, a, b, float(a) - b)  # exact: no tolerance on integer columns
            else:
                assert bits(a) == bits(b), (k, fn, col, a, b)


# ------------------------------------------------------------------ CPU tests of the reference itself
def test_reference_float_of_int_rounds_to_nearest_even():
    assert float(2 ** 53 + 1) == 2.0 ** 53
    assert float(2 ** 53 + 3) == 2.0 ** 53 + 4
    assert float(-(2 ** 53 + 1)) == -(2.0 ** 53) and float(-(2 ** 53 + 3)) == -(2.0 ** 53 + 4)
    assert float(2 ** 54 - 1) == 2.0 ** 54  # the carry into the next binade
    assert float((2 ** 53 - 1) * 2 ** 11 + 2 ** 10) == 2.0 ** 64
    assert float((2 ** 53 + 1) * 2 ** 11 + 2 ** 10 + 1) == float((2 ** 53 + 2) * 2 ** 11)  # tie + sticky: up
    assert float(2 ** 66 + 2 ** 13) == 2.0 ** 66


def test_reference_split_sums_against_a_plain_loop():
    rng = np.random.default_rng(3)
    v = rng.integers(I64_MIN, I64_MAX, size=5000, dtype=np.int64, endpoint=True)
    v[:4] = [I64_MIN, I64_MAX, -1, 0xffffffff]
    inv = rng.integers(0, 7, size=len(v))
    want = [0] * 7
    for x, g in zip(v.tolist(), inv.tolist()):
        want[g] += x
    assert exact_group_sums(v, inv, 7) == want
    assert max(abs(w) for w in want) > 1 << 64


def test_reference_designed_groups_hit_their_targets():
    d = designed_docs()
    for gid, (name, total) in enumerate(TARGETS):
        vals = [v for g, v in zip(d["g"], d["v"]) if g == gid]
        assert sum(vals) == total and all(I64_MIN <= v <= I64_MAX for v in vals), name
        if abs(total) <= 1 and name.startswith("cancel"):
            assert max(abs(v) for v in vals) > 1 << 61
    cols = {"g": np.array(d["g"]), "v": np.array(d["v"], dtype=np.int64)}
    ref = reference(cols, {"g": "INT", "v": "LONG"}, None, ["g"], [("COUNT", None), ("SUM", "v"), ("MIN", "v")])
    for gid, (name, total) in enumerate(TARGETS):
        assert ref[(gid,)][1] == float(total), name
    assert ref[(GID["int64_min"],)] == [1, -2.0 ** 63, -2.0 ** 63]


def test_reference_double_sum_rules():
    assert DoubleSum([1.0, math.inf, -3.0]).matches(math.inf) and not DoubleSum([1.0, math.inf]).matches(1.0)
    assert DoubleSum([math.inf, -math.inf]).matches(math.nan) and not DoubleSum([math.inf, -math.inf]).matches(math.inf)
    assert DoubleSum([0.1] * 10).matches(sum([0.1] * 10)) and not DoubleSum([0.1] * 10).matches(1.0 + 1e-13)


# ------------------------------------------------------------------ designed groups
def _targets():
    t = []
    for name, x in (("tie_down_2^53+1", 2 ** 53 + 1), ("tie_up_2^53+3", 2 ** 53 + 3), ("binade_2^54-1", 2 ** 54 - 1),
                    ("binade_carry_2^64", (2 ** 53 - 1) * 2 ** 11 + 2 ** 10),
                    ("tie_sticky", (2 ** 53 + 1) * 2 ** 11 + 2 ** 10 + 1), ("2^63", 2 ** 63), ("2^64", 2 ** 64),
                    ("2^64+1", 2 ** 64 + 1), ("2^64-1", 2 ** 64 - 1), ("2^66+2^13", 2 ** 66 + 2 ** 13)):
        t += [("+" + name, x), ("-" + name, -x)]
    t += [("cancel_0", 0), ("cancel_1", 1), ("cancel_-1", -1)]
    # (filled by designed_docs, not by parts(): the values are the point)
    t += [("low_crosses_2^32_high_negative", 3 * (-5 * 2 ** 32 + 0xfffffff0)), ("int64_min", I64_MIN),
          ("int64_max", I64_MAX), ("int64_min_and_max", -1)]
    return t


TARGETS = _targets()
GID = {name: i for i, (name, _) in enumerate(TARGETS)}
NG = len(TARGETS)
# double specials live in the first groups (g < NSPECIAL), so that `g >= NSPECIAL` is a dense filter over ordinary doubles
SPECIAL_D = [[math.inf, 1.5, -2.5e7], [-math.inf, -1.0, 3.25], [math.inf, -math.inf, 7.0],
             [5e-324, -5e-324, DBL_MAX, -DBL_MAX], [-5e-324, -1e-300, -2.5], [5e-324, 1e-300],
             [FLT_MAX, -FLT_MAX, FLT_SUB, -FLT_SUB], [-1e300, -3.0]]
SPECIAL_F = [[math.inf, 1.5, -2.5e7], [-math.inf, -1.0, 3.25], [math.inf, -math.inf, 7.0],
             [FLT_SUB, -FLT_SUB, FLT_MAX, -FLT_MAX], [-FLT_SUB, -1e-30, -2.5], [FLT_SUB, 1e-30],
             [FLT_MAX, -1.0], [-FLT_MAX, -3.0]]
NSPECIAL = len(SPECIAL_D)


def parts(total, rng):
    """LONG values that add up exactly to `total`: steps of about +/-2^62 towards it, three pairs near +/-2^62 that
    cancel, and the remainder."""
    vals, rem = [], total
    while abs(rem) > 1 << 62:
        step = (1 << 62) - int(rng.integers(0, 1 << 20))
        step = step if rem > 0 else -step
        vals.append(step)
        rem -= step
    for _ in range(3):
        a = int(rng.integers(1 << 61, 1 << 62))
        vals += [a, -a]
    vals.append(rem)
    order = rng.permutation(len(vals))
    return [vals[i] for i in order]


def designed_docs():
    """The designed docs as column lists, sorted by group: g (group id), v (LONG), d (DOUBLE), f (FLOAT values)."""
    rng = np.random.default_rng(2024)
    out = {"g": [], "v": [], "d": [], "f": []}
    for gid, (name, total) in enumerate(TARGETS):
        if name == "low_crosses_2^32_high_negative":
            vals = [-5 * 2 ** 32 + 0xfffffff0] * 3
        elif name == "int64_min":
            vals = [I64_MIN]
        elif name == "int64_max":
            vals = [I64_MAX]
        elif name == "int64_min_and_max":
            vals = [I64_MAX, I64_MIN]
        else:
            vals = parts(total, rng)
        n = len(vals)
        if gid < NSPECIAL:
            assert n >= 4
            ds = SPECIAL_D[gid] + [-1234.5] * (n - len(SPECIAL_D[gid]))
            fs = SPECIAL_F[gid] + [-1234.5] * (n - len(SPECIAL_F[gid]))
        else:
            ds = np.round(rng.normal(-10, 1e6, size=n), 3).tolist()
            fs = rng.normal(-10, 1e3, size=n).astype(np.float32).astype(np.float64).tolist()
        out["g"] += [gid] * n
        out["v"] += vals
        out["d"] += ds
        out["f"] += fs
    return out


SCHEMA = {"g": "INT", "k1": "INT", "k2": "INT", "f": "INT", "v": "LONG", "vd": "LONG", "vn": "LONG", "va": "LONG",
          "ri": "INT", "rd": "DOUBLE", "dd": "DOUBLE", "rf": "FLOAT", "rg": "INT", "rk": "LONG"}
RAW = ("v", "ri", "rd", "rf", "rg", "rk")
NFILL_GROUPS = 300
HOT_VALUE = (1 << 62) - 3     # low 32 bits 0xfffffffd: count * low32 passes 2^32 at the second doc
VA_BASE, VA_STEP, VA_CARD = -(1 << 62) + 1, (1 << 20) + 1, 1000
VN_BIG = 1 << 45
HOT_KEY = (200, 200)          # 700 docs of vn ~ -2^45: a per-key total of about -2^54.5


def _columns(n_fill, seed):
    """The designed docs scattered among n_fill filler docs (n_fill = 0: the designed docs alone, sorted by group).
    Filler docs never share a key with a designed group: g >= NG, k1 >= 64."""
    rng = np.random.default_rng(seed)
    d = designed_docs()
    nd = len(d["g"])
    n = nd + n_fill
    pos = np.sort(rng.choice(n, size=nd, replace=False)) if n_fill else np.arange(nd)
    fill = np.ones(n, dtype=bool)
    fill[pos] = False
    nf = n_fill
    pool = np.unique(rng.integers(-(1 << 62), 1 << 62, size=1500))
    c = {}
    c["g"] = np.empty(n, dtype=np.int32)
    c["g"][pos] = d["g"]
    c["g"][fill] = NG + rng.integers(0, NFILL_GROUPS, size=nf)
    c["k1"] = np.empty(n, dtype=np.int32)
    c["k2"] = np.empty(n, dtype=np.int32)
    c["k1"][pos] = d["g"]
    c["k2"][pos] = 255 - np.array(d["g"])
    c["k1"][fill] = rng.integers(64, 256, size=nf)
    c["k2"][fill] = rng.integers(0, 256, size=nf)
    # f: 0 on the first eight designed groups (about 0.02 % of a filled segment), 1 on the others, 2.. on filler docs
    c["f"] = np.empty(n, dtype=np.int32)
    c["f"][pos] = (np.array(d["g"]) >= 8).astype(np.int32)
    c["f"][fill] = rng.integers(2, 4000, size=nf)
    v = np.empty(n, dtype=np.int64)
    v[pos] = d["v"]
    fv = pool[rng.integers(0, len(pool), size=nf)]
    fv[rng.random(nf) < 0.2] = HOT_VALUE
    v[fill] = fv
    c["v"] = v
    c["vd"] = v.copy()
    # vn: |values| <= 2^45 exactly (v_maxabs = 2^45)
    npool = np.concatenate([[-VN_BIG, -VN_BIG + 1, -VN_BIG + 2, VN_BIG - 7, VN_BIG], rng.integers(-(1 << 44), 1 << 44, 900)])
    c["vn"] = npool[rng.integers(0, len(npool), size=n)].astype(np.int64)
    c["va"] = (VA_BASE + VA_STEP * rng.integers(0, VA_CARD, size=n)).astype(np.int64)
    c["ri"] = rng.integers(I32_MIN, I32_MAX, size=n, endpoint=True).astype(np.int32)
    c["ri"][pos[:2]] = [I32_MIN, I32_MAX]
    dpool = np.unique(np.round(rng.normal(-10, 1e6, size=3000), 3))  # (a dictionary small enough for LDS tables)
    rd = dpool[rng.integers(0, len(dpool), size=n)]
    rd[pos] = d["d"]
    c["rd"] = rd
    c["dd"] = rd.copy()
    rf = rng.normal(-10, 1e3, size=n).astype(np.float32)
    rf[pos] = np.array(d["f"], dtype=np.float64).astype(np.float32)
    c["rf"] = rf
    if n_fill:
        hot = np.flatnonzero(fill)[:700]
        c["k1"][hot], c["k2"][hot] = HOT_KEY
        c["g"][hot] = NG + NFILL_GROUPS
        c["vn"][hot] = -VN_BIG + (np.arange(len(hot)) % 3)
        c["va"][np.flatnonzero(fill)[700:700 + VA_CARD]] = VA_BASE + VA_STEP * np.arange(VA_CARD)  # every value occurs
    c["rg"] = c["g"].copy()
    c["rk"] = c["k1"].astype(np.int64) * 256 + c["k2"]
    return c


class Table:
    count = 0

    def __init__(self, name, cols_list, schema=SCHEMA, raw=RAW, mv=()):
        Table.count += 1
        self.uid = Table.count
        self.schema = schema
        self.segs = [create_segment("%s%d" % (name, i), c, schema, no_dictionary_columns=raw, multi_value_columns=mv)
                     for i, c in enumerate(cols_list)]
        self.cols = {k: np.concatenate([np.asarray(c[k]) for c in cols_list]) for k in schema if k not in mv}
        self.gs = None

    def open(self):
        self.gs = [GpuSegment(s) for s in self.segs]
        return self

    def close(self):
        for g in self.gs or []:
            g.close()


N_FILL = 150_000


@pytest.fixture(scope="module")
def filled():
    """The designed docs among 150k filler docs, one segment (every dictionary shared when bound twice)."""
    t = Table("filled", [_columns(N_FILL, 7)]).open()
    yield t
    t.close()


@pytest.fixture(scope="module")
def bare():
    """The designed docs alone, sorted by group (a wave's docs share a few keys)."""
    t = Table("bare", [_columns(0, 8)]).open()
    yield t
    t.close()


def parse_aggs(text):
    out = []
    for a in text.split(","):
        fn, col = a.strip().rstrip(")").split("(")
        out.append((fn, None if col == "*" else col))
    return out


MASKS = {
    None: lambda c: None,
    "f < 1": lambda c: c["f"] < 1,
    "f >= 1": lambda c: c["f"] >= 1,
    "f < 4000": lambda c: c["f"] < 4000,
    "g >= %d" % NSPECIAL: lambda c: c["g"] >= NSPECIAL,
    "g < %d" % NSPECIAL: lambda c: c["g"] < NSPECIAL,
    "g = 3": lambda c: c["g"] == 3,
    "g = 6": lambda c: c["g"] == 6,
}
DENSE_ORDINARY = "g >= %d" % NSPECIAL
_REF_CACHE = {}


def run_case(table, aggs, group_by=(), where=None, flags=0, tuning=None, plan=None, bind=1):
    """Runs the query, asserts the plan (plan: {stats()["plan"] key: value or predicate}) and compares with the
    reference over the same docs. bind: how many times the table's segments are bound."""
    group_by = list(group_by)
    sql = "SELECT %s FROM t" % ", ".join(group_by + [aggs])
    if where:
        sql += " WHERE " + where
    if group_by:
        sql += " GROUP BY %s LIMIT 10000000 OPTION(numGroupsLimit=10000000)" % ", ".join(group_by)
    q = parse_sql(sql)
    ex = GpuQueryExecutor(q, table.gs * bind, flags=flags, tuning=tuning)
    try:
        st = ex.stats()["plan"]
        for key, want in (plan or {}).items():
            ok = want(st[key]) if callable(want) else st[key] == want
            assert ok, (sql, key, st)
        got = ex.run()
    finally:
        ex.close()
    al = parse_aggs(aggs)
    ck = (table.uid, bind, aggs, tuple(group_by), where)
    if ck not in _REF_CACHE:
        _REF_CACHE[ck] = reference(table.cols, table.schema, MASKS[where](table.cols), group_by, al, times=bind)
    assert_matches(got, _REF_CACHE[ck], al, table.schema, group_by)
    return got, st


def assert_designed(got, key_of=lambda gid: (gid,), sum_at=1):
    """The designed groups came back with float(target) — stated once more against TARGETS themselves."""
    for gid, (name, total) in enumerate(TARGETS):
        assert got.groups[key_of(gid)][sum_at] == float(total), (name, got.groups[key_of(gid)], float(total))


LONG_AGGS = "COUNT(*), SUM(v), MIN(v), MAX(v)"
DICT_AGGS = "COUNT(*), SUM(vd), MIN(vd), MAX(vd)"


# ------------------------------------------------------------------ aggregation-only paths
@pytest.mark.gpu
@pytest.mark.parametrize("where", [None, "f >= 1", "f < 1", DENSE_ORDINARY, "g = 6"])
@pytest.mark.parametrize("aggs", [LONG_AGGS, "SUM(ri), MIN(ri), MAX(ri), SUM(v)", "SUM(rd), MIN(rd), MAX(rd)",
                                  "SUM(rf), MIN(rf), MAX(rf), COUNT(*)"])
def test_lane_raw_lane_major(filled, aggs, where):
    """Per-lane registers over raw columns, lane-major: dense tiles (no filter, ~100 %), sparse tiles (0.02 %)."""
    run_case(filled, aggs, where=where, plan={"strategy": "lane", "variant": "lane_raw", "lane_major": 1})


@pytest.mark.gpu
@pytest.mark.parametrize("where", [None, "f >= 1", "f < 1"])
@pytest.mark.parametrize("flags", [0, L.PA_QF_NO_LANE_HIST])
def test_lane_dict_histogram_fold(filled, where, flags):
    """lane_dict: SUM over a dictionary (at most 16384 values) bound twice — dictId counts folded in as count * low32 and
    count * (v >> 32); HOT_VALUE near 2^62 is hit by a fifth of the docs. Also the per-doc gather (PA_QF_NO_LANE_HIST)
    and the dictionary DOUBLE column."""
    assert len(filled.segs[0].column("vd").dictionary) <= 16384
    plan = {"strategy": "lane", "variant": "lane_dict", "lane_major": 1}
    run_case(filled, DICT_AGGS, where=where, flags=flags, plan=plan, bind=2)
    run_case(filled, "SUM(vd), SUM(vn), SUM(va)", where=where, flags=flags, plan=plan, bind=2)
    run_case(filled, "SUM(dd), MIN(dd), MAX(dd)", where=where if where else DENSE_ORDINARY, flags=flags, plan=plan, bind=2)


@pytest.mark.gpu
@pytest.mark.parametrize("where", [None, "f < 1"])
def test_lane_step_major(filled, where):
    plan = {"strategy": "lane", "lane_major": 0}
    run_case(filled, LONG_AGGS, where=where, flags=L.PA_QF_NO_LANE_MAJOR, plan=plan)
    run_case(filled, DICT_AGGS, where=where, flags=L.PA_QF_NO_LANE_MAJOR, plan=plan)
    run_case(filled, "SUM(rd), MIN(rd), MAX(dd), MIN(rf)", where=where, flags=L.PA_QF_NO_LANE_MAJOR, plan=plan)


@pytest.mark.gpu
@pytest.mark.parametrize("strategy,flags", [("lds", L.PA_QF_NO_LANE_ACC),
                                            ("global", L.PA_QF_NO_LANE_ACC | L.PA_QF_FORCE_GLOBAL)])
@pytest.mark.parametrize("major", [0, L.PA_QF_NO_LANE_MAJOR])
def test_aggregation_only_lds_and_global(filled, bare, strategy, flags, major):
    """Aggregation-only on the workgroup's LDS accumulators and on the global ones (accumulate / update_one /
    lds_update with a single key)."""
    plan = {"strategy": strategy}
    for aggs in (LONG_AGGS, DICT_AGGS, "SUM(ri), MIN(ri), MAX(ri)"):
        run_case(filled, aggs, flags=flags | major, plan=plan)
        run_case(bare, aggs, flags=flags | major, plan=plan)
    run_case(filled, "SUM(rd), MIN(rd), MAX(rd), MIN(rf), MAX(dd)", where=DENSE_ORDINARY, flags=flags | major, plan=plan)
    run_case(bare, "SUM(rd), MIN(rd), MAX(rd), MIN(rf), MAX(rf), MIN(dd), MAX(dd)", flags=flags | major, plan=plan)


# ------------------------------------------------------------------ GROUP BY in LDS and in global memory
@pytest.mark.gpu
@pytest.mark.parametrize("where", [None, "f >= 1", "f < 1"])
@pytest.mark.parametrize("major", [1, 0])
def test_group_by_lds(filled, where, major):
    """GROUP BY over a few hundred keys on the LDS strategy, lane-major (accumulate_lds_lm; accumulate_lds_raw_dense
    when every aggregation reads one raw LONG column and the tile is dense) and step-major."""
    flags = L.PA_QF_NO_DENSE_GROUP | (0 if major else L.PA_QF_NO_LANE_MAJOR)
    if where == "f < 1":  # (the planner keeps a sparse filter's survivors on the global accumulators unless told)
        flags |= L.PA_QF_FORCE_LDS
    plan = {"strategy": "lds", "lane_major": major}
    got, _ = run_case(filled, LONG_AGGS, ["g"], where, flags=flags, plan=plan)  # one raw LONG column: raw-dense
    if where is None:
        assert_designed(got)
    got, _ = run_case(filled, "COUNT(*), SUM(vd), MIN(vd), MAX(v), SUM(ri)", ["g"], where, flags=flags, plan=plan)
    if where is None:
        assert_designed(got)
    run_case(filled, "SUM(rd), MIN(rd), MAX(rd), MIN(rf), MAX(rf), MIN(dd), MAX(dd)", ["g"], where, flags=flags, plan=plan)


@pytest.mark.gpu
@pytest.mark.parametrize("major", [0, L.PA_QF_NO_LANE_MAJOR])
def test_group_by_global_grouped_and_ungrouped(filled, bare, major):
    """The global strategy's wave pre-reduction: docs sorted by group (a wave's docs share a few keys: one leader adds
    the wave's partial sums) and 56064 keys at random (every doc its own atomics)."""
    flags = L.PA_QF_FORCE_GLOBAL | major
    plan = {"strategy": "global"}
    for aggs in (LONG_AGGS, DICT_AGGS):
        got, _ = run_case(bare, aggs, ["g"], flags=flags, plan=plan)
        assert_designed(got)
        got, _ = run_case(filled, aggs, ["k1", "k2"], flags=flags, plan=plan)
        assert_designed(got, key_of=lambda gid: (gid, 255 - gid))
    run_case(bare, "SUM(rd), MIN(rd), MAX(rd), MIN(rf), MAX(rf), SUM(dd)", ["g"], flags=flags, plan=plan)
    run_case(filled, "SUM(rd), MIN(rd), MAX(rd), MIN(rf), MAX(rf)", ["g"], flags=flags, plan=plan)


# ------------------------------------------------------------------ dense GROUP BY (staged columns)
@pytest.mark.gpu
@pytest.mark.parametrize("mode,flags", [("step", L.PA_QF_NO_GDENSE_LM), ("lm_unpacked", L.PA_QF_NO_GD_PACK), ("default", 0)])
def test_group_by_dense(filled, mode, flags):
    """The staged-column GROUP BY kernel: raw LONG (the split pair), a dictionary beyond int32 (GOP_SUM_L over a value
    table), the affine dictionary (GVS_ID: gd_flush's base * count + step * sum needs its 128 bits with the base near
    -2^62), doubles; step-major, lane-major with one atomic per aggregation, and the planner's own choice."""
    raw = {"strategy": "lds_dense", "dense_packed": (lambda p: True) if mode == "default" else 0}
    if mode == "step":
        raw["variant"] = lambda v: not v.startswith("gdense_lm")
    # (a 64-bit raw column can leave no room for two tile images per wave: a step-major variant then runs, so the
    # lane-major walk is asserted on the dictionary columns' queries)
    plan = dict(raw, variant=lambda v: v.startswith("gdense_lm")) if mode == "lm_unpacked" else raw
    for where in ("f < 4000", "f >= 1"):
        got, _ = run_case(filled, LONG_AGGS, ["g"], where, flags=flags, plan=raw)
        if where == "f < 4000":
            assert_designed(got)
        got, _ = run_case(filled, "COUNT(*), SUM(vd), MIN(vd), MAX(vd)", ["g"], where, flags=flags, plan=plan)
        if where == "f < 4000":
            assert_designed(got)
        run_case(filled, "SUM(va), COUNT(*), MIN(va)", ["g"], where, flags=flags, plan=plan)
        run_case(filled, "SUM(rd), MIN(rd), MAX(rd), MIN(rf)", ["g"], where, flags=flags, plan=raw)
        run_case(filled, "SUM(dd), MIN(dd), MAX(dd), MAX(vd)", ["g"], where, flags=flags, plan=plan)


# ------------------------------------------------------------------ partitioned aggregation (pass C)
# narrow: pass C keeps a partition's 64-bit SUM in one word when records < 2^62 / v_maxabs. vn's largest magnitude is
# 2^45, so the bound is 2^62 / 2^45 = 2^17 = 131072 records per partition. The planner halves the partitions' key range
# until there are kMinParts = 256 of them or they are down to 256 keys (the count-free emit: one partition per CU), so
# the 56064 keys make about 219 partitions of about 150k / 219 = 700 records, 1400 where the hot key's 700 docs fall:
# two orders of magnitude below the bound, so every partition takes the one-word form. vd and va reach 2^62: their bound
# is 1 record, which no partition with records meets, so they take the split pair.
PART_CASES = {
    "generic_two_sums": ("COUNT(*), SUM(vd), SUM(vn)", False),
    "id_wide": (DICT_AGGS, True),
    "id_narrow": ("COUNT(*), SUM(vn), MIN(vn), MAX(vn)", True),
    "id_affine": ("COUNT(*), SUM(va), MIN(va), MAX(va)", True),
    "raw_long": (LONG_AGGS, True),
    "raw_int": ("COUNT(*), SUM(ri), MIN(ri), MAX(ri)", True),
    "raw_double": ("SUM(rd), MIN(rd), MAX(rd)", True),
    "dict_double": ("SUM(dd), MIN(dd), MAX(dd)", True),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case,count_free", [(c, cf) for c in PART_CASES for cf in (0, 1) if cf == 0 or PART_CASES[c][1]])
def test_partitioned(filled, case, count_free):
    """Pass C of the partitioned aggregation, with the count pass and with the count-free emit (the generic pass C of
    several payloads has no count-free emit)."""
    aggs, _ = PART_CASES[case]
    plan = {"strategy": "partitioned", "count_free_emit": count_free}
    got, _ = run_case(filled, aggs, ["k1", "k2"], flags=0 if count_free else L.PA_QF2_NO_COUNT_FREE, plan=plan)
    if case in ("id_wide", "raw_long", "generic_two_sums"):
        assert_designed(got, key_of=lambda gid: (gid, 255 - gid))
    if case == "id_narrow":  # a negative per-key total past 2^53 from the one-word form
        assert got.groups[HOT_KEY][1] < -(2.0 ** 54) and got.groups[HOT_KEY][0] >= 700


# ------------------------------------------------------------------ the device-side final rounding
@pytest.mark.gpu
@pytest.mark.parametrize("flags,strategy", [(L.PA_QF_NO_PARTITION, "global"), (0, "partitioned")])
def test_direct_key_space_block_over_1mib(filled, flags, strategy):
    """GROUP BY a 219-value and a 256-value column: 56064 keys x (count + the 96-bit SUM pair + MIN + MAX) = 2.2 MB of
    accumulators,
    past kFetchWholeBlockBytes, so compact_final_kernel converts on the device: sum_pair_to_i128 + i128_to_double for
    the SUM, i128_to_double for the int64 MIN / MAX (INT64_MIN and INT64_MAX among them). Every designed target."""
    got, st = run_case(filled, LONG_AGGS, ["k1", "k2"], flags=flags, plan={"strategy": strategy})
    assert len(got.groups) > 30000
    assert_designed(got, key_of=lambda gid: (gid, 255 - gid))
    assert got.groups[(GID["int64_min"], 255 - GID["int64_min"])] == [1, -2.0 ** 63, -2.0 ** 63, -2.0 ** 63]
    assert got.groups[(GID["int64_max"], 255 - GID["int64_max"])] == [1, 2.0 ** 63, 2.0 ** 63, 2.0 ** 63]
    assert got.groups[(GID["int64_min_and_max"], 255 - GID["int64_min_and_max"])] == [2, -1.0, -2.0 ** 63, 2.0 ** 63]
    # int64 SUM (an INT column) and COUNT-only rows through the same kernel
    run_case(filled, "SUM(ri), MIN(ri), MAX(ri), SUM(vd), MIN(rd), MAX(rd)", ["k1", "k2"], flags=flags)


@pytest.mark.gpu
def test_hashed_key_space(filled, bare):
    """GROUP BY raw columns (hashed key space): the host decode of a small block and of one past 1 MiB."""
    got, _ = run_case(bare, LONG_AGGS, ["rg"])
    assert_designed(got)
    got, _ = run_case(filled, DICT_AGGS, ["rg"])
    assert_designed(got)
    got, _ = run_case(filled, LONG_AGGS, ["rk"])
    assert len(got.groups) > 30000
    assert_designed(got, key_of=lambda gid: (gid * 256 + 255 - gid,))


# ------------------------------------------------------------------ multi-value LONG column
@pytest.mark.gpu
def test_mv_long_sum_min_max():
    """SUMMV / MINMV / MAXMV over a LONG multi-value column: each designed group's values as the entries of its docs."""
    d = designed_docs()
    rng = np.random.default_rng(5)
    gids, entries = [], []
    for gid in range(NG):
        vals = [v for g, v in zip(d["g"], d["v"]) if g == gid]
        while vals:
            k = int(rng.integers(1, 4))
            gids.append(gid)
            entries.append(np.array(vals[:k], dtype=np.int64))
            vals = vals[k:]
    seg = create_segment("mv", {"g": np.array(gids, dtype=np.int32), "mv": entries}, {"g": "INT", "mv": "LONG"},
                         multi_value_columns=("mv",))
    gs = GpuSegment(seg)
    try:
        for group_by in ([], ["g"]):
            sql = "SELECT %sCOUNT(*), SUMMV(mv), MINMV(mv), MAXMV(mv) FROM t%s" % (
                "g, " if group_by else "", " GROUP BY g LIMIT 1000" if group_by else "")
            ex = GpuQueryExecutor(parse_sql(sql), [gs], flags=L.PA_QF_FORCE_GLOBAL)
            try:
                assert ex.stats()["plan"]["strategy"] == "global"
                got = ex.run()
            finally:
                ex.close()
            flat_g = np.concatenate([[g] * len(e) for g, e in zip(gids, entries)])
            cols = {"g": flat_g, "mv": np.concatenate(entries)}
            want = reference(cols, {"g": "INT", "mv": "LONG"}, None, group_by, [("SUM", "mv"), ("MIN", "mv"), ("MAX", "mv")])
            if group_by:
                assert set(got.groups) == set(want)
                for k, w in want.items():
                    assert [float(x) for x in got.groups[k][1:]] == w, (k, got.groups[k], w)
                    assert got.groups[k][1] == float(TARGETS[k[0]][1])
            else:
                assert [float(x) for x in got.row[1:]] == want[()], (got.row, want[()])
    finally:
        gs.close()


# ------------------------------------------------------------------ the int32 boundary of a dictionary
@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, L.PA_QF_NO_DENSE_GROUP, L.PA_QF_FORCE_GLOBAL])
def test_dictionary_leaving_int32_in_one_segment(flags):
    """A dictionary LONG column whose values fit int32 in one segment (INT32_MIN and INT32_MAX among them) and leave it
    by one in the other: SUM / MIN / MAX per group exact, and equal to the two segments' own results combined."""
    rng = np.random.default_rng(9)
    n = 20_011
    schema = {"g": "INT", "m": "LONG"}
    pool_a = np.concatenate([[I32_MIN, I32_MAX, I32_MIN + 1, I32_MAX - 1], rng.integers(I32_MIN, I32_MAX, 500)])
    pool_b = np.concatenate([pool_a, [I32_MAX + 1, I32_MIN - 1]])
    cols = []
    for pool in (pool_a, pool_b):
        m = pool[rng.integers(0, len(pool), size=n)].astype(np.int64)
        m[:len(pool)] = pool
        g = rng.integers(0, 40, size=n).astype(np.int32)
        g[m > I32_MAX] = 0           # group 0: INT32_MAX + 1 and INT32_MAX, group 1: INT32_MIN - 1 and INT32_MIN
        g[m < I32_MIN] = 1
        g[m == I32_MAX] = 0
        g[m == I32_MIN] = 1
        cols.append({"g": g, "m": m})
    aggs = "COUNT(*), SUM(m), MIN(m), MAX(m)"
    both = Table("edge", cols, schema, raw=()).open()
    singles = [Table("edge%d" % i, [c], schema, raw=()).open() for i, c in enumerate(cols)]
    try:
        for where, mask in ((None, lambda c: None), ("g < 2", lambda c: c["g"] < 2)):
            MASKS.setdefault(where, mask)
            for group_by in (["g"], []):
                got, _ = run_case(both, aggs, group_by, where, flags=flags)
                parts_ = [run_case(t, aggs, group_by, where, flags=flags)[0] for t in singles]
                rows = [p.groups if group_by else {(): p.row} for p in parts_]
                mine = got.groups if group_by else {(): got.row}
                ref = reference(both.cols, schema, mask(both.cols), group_by, parse_aggs(aggs))
                for k, row in mine.items():
                    have = [r[k] for r in rows if k in r]
                    # (SUM: per-segment totals here stay below 2^53, so their doubles add exactly)
                    assert row == [sum(h[0] for h in have), sum(h[1] for h in have), min(h[2] for h in have),
                                   max(h[3] for h in have)], (k, row, have)
                    assert ref[k][1] == row[1]
                if group_by and where is None:
                    assert mine[(0,)][3] == float(I32_MAX + 1) and mine[(1,)][2] == float(I32_MIN - 1)
    finally:
        both.close()
        for t in singles:
            t.close()


# ------------------------------------------------------------------ a hot key at the packed fields' capacity
HOT_N = 700_000  # docs per segment; two segments on one workgroup: 16 waves of about 85 tiles of 1024 docs each


def _hot_table(shape, own):
    """Two segments whose docs all hold the dictionary's largest value (m, m2) or its smallest (mz, m2z: every packed
    term is 0), in one group (g1; its last doc alone in a second one, so the column has a bit) or alternating between
    two (g2). own: the second segment's dictionary has one more value (tables of offsets from the minimum instead of
    the shared dictionary's ids)."""
    s = HOT_SHAPES[shape]
    cols = []
    for si in range(2):
        n = s["docs"] + 13 * si
        c = {"f": np.zeros(n, dtype=np.int32), "g1": np.zeros(n, dtype=np.int32),
             "g2": (np.arange(n) % 2).astype(np.int32)}
        c["f"][-1] = c["g1"][-1] = 1
        for name, key, key_own in (("m", "dict_a", "dict_b"), ("m2", "second", "second_b")):
            d = np.array(s.get(key_own, s[key]) if (own and si) else s[key], dtype=np.int64)
            for suffix, fill in (("", d.max()), ("z", d.min())):
                m = np.full(n, fill, dtype=np.int64)
                m[:len(d)] = d  # every dictionary value occurs
                c[name + suffix] = m
        cols.append(c)
    schema = {"f": "INT", "g1": "INT", "g2": "INT", "m": "LONG", "mz": "LONG", "m2": "LONG", "m2z": "LONG"}
    return Table("hot", cols, schema, raw=())


HOT_SHAPES = {
    # one SUM over {lo, lo + 2^32 - 1}: own dictionaries give 32-bit offsets, w = 32, c = (64 - 32) / 2 = 16 (a shared
    # two-value dictionary is affine: its dictIds are the terms, w = 1 and c = 31). The generic packed kernel takes
    # value tables of int32 values only (GOP_SUM_I), so without the JIT the own-dictionary forms of the two 64-bit
    # shapes run unpacked (nojit_own_packed = False); w32_int32 is the nearest shape it accepts at w = 32, c = 16
    "w32_int32": dict(dict_a=[I32_MIN, I32_MAX], dict_b=[I32_MIN, I32_MIN + 5, I32_MAX], second=[0, 1], docs=HOT_N,
                      aggs="COUNT(*), SUM(m)"),
    "w32_low": dict(dict_a=[-(1 << 40), -(1 << 40) + (1 << 32) - 1], second=[0, 1], docs=HOT_N,
                    dict_b=[-(1 << 40), -(1 << 40) + 5, -(1 << 40) + (1 << 32) - 1], aggs="COUNT(*), SUM(m)",
                    nojit_own_packed=False),
    "w32_high": dict(dict_a=[I64_MAX - (1 << 32), I64_MAX - 1], second=[0, 1], docs=HOT_N,
                     dict_b=[I64_MAX - (1 << 32), I64_MAX - (1 << 32) + 5, I64_MAX - 1], aggs="COUNT(*), SUM(m)",
                     nojit_own_packed=False),
    # two SUMs with spans 2^16 - 1 and 2^15 - 1 (own dictionaries: offsets): w = 16 + 15, c = (64 - 31) / 3 = 11, the
    # smallest field (2047 docs, drained after every tile), and 31 + 3 * 11 = 64: no spare bit above COUNT, which
    # spans 2^15 - 1 twice would leave. (Shared two-value dictionaries are affine: w = 1 + 1, c = 20.)
    "w16_w15": dict(dict_a=[-7, -7 + (1 << 16) - 1], dict_b=[-7, -3, -7 + (1 << 16) - 1], docs=100_000,
                    second=[1000, 1000 + (1 << 15) - 1], second_b=[1000, 1003, 1000 + (1 << 15) - 1],
                    aggs="COUNT(*), SUM(m), SUM(m2)"),
    # COUNT(*) alone: the field is capped at c = 31
    "count_only": dict(dict_a=[1, 2], dict_b=[1, 2, 3], second=[0, 1], docs=100_000, aggs="COUNT(*)"),
}


@pytest.fixture(scope="module")
def hot_tables():
    cache = {}

    def get(shape, own):
        if (shape, own) not in cache:
            cache[(shape, own)] = _hot_table(shape, own).open()
        return cache[(shape, own)]

    yield get
    for t in cache.values():
        t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("jit", [1, 0])
@pytest.mark.parametrize("own", [0, 1])
@pytest.mark.parametrize("shape", list(HOT_SHAPES))
def test_hot_key_at_packed_capacity(hot_tables, shape, own, jit):
    """Every doc in one group and every term the largest: a packed field fills as fast as it can, so a drain period one
    tile too long overflows it. One workgroup (scan_grid = 1) so that each wave runs more tiles than a drain period
    (c = 16: 63 tiles; c = 11: one). Then every term 0 (all-minimum values), then two groups alternating."""
    flags = 0 if jit else L.PA_QF_NO_JIT
    packed = 2 if jit else 1 if (not own or HOT_SHAPES[shape].get("nojit_own_packed", True)) else 0
    plan = {"strategy": "lds_dense", "dense_packed": packed}
    t = hot_tables(shape, own)
    aggs = HOT_SHAPES[shape]["aggs"]
    for g, a, where in (("g1", aggs, "f < 4000"), ("g1", aggs, "f < 1"),
                        ("g1", aggs.replace("m)", "mz)").replace("m2)", "m2z)"), "f < 1"), ("g2", aggs, "f < 1")):
        run_case(t, a, [g], where, flags=flags, tuning={"scan_grid": 1}, plan=plan)
    if jit and own and shape == "w16_w15":
        # The specialised kernel sizes its own grid (one workgroup per CU at most), keeps one row replica per lane while
        # they fit, and then drains every (2^c - 1) / ND tiles: far more than a wave ever runs. With one replica
        # (gdl_rr = 1: what many keys per segment leave room for) a c = 11 row holds two 1024-doc tiles less one doc, so
        # it drains after every tile; the segments bound 16 times (3.2M docs) give the 8-wave workgroups' waves two
        # tiles each. Rows shared by two waves (gdl_rs = 2) take both waves' tiles: with 512-doc tiles (gdl_nd = 8) the
        # period is 2047 / 512 / 2 = 1 tile; with 1024-doc tiles it would be 0 — two tiles are 2048 docs, one more than
        # the field holds — so the planner has to decline that candidate (the generic packed kernel runs: 1).
        for tuning, packed in (({"gdl_rr": 1, "gdl_w": 8, "gdl_nd": 16}, 2), ({"gdl_rr": 1, "gdl_rs": 2, "gdl_nd": 8}, 2),
                               ({"gdl_rr": 1, "gdl_rs": 2, "gdl_nd": 16}, 1)):
            run_case(t, aggs, ["g1"], "f < 4000", tuning=tuning, plan=dict(plan, dense_packed=packed), bind=16)


# ------------------------------------------------------------------ doubles at the ends of the order encoding
@pytest.mark.gpu
@pytest.mark.parametrize("where", ["g < %d" % NSPECIAL, "g = 3", "g = 6", None])
def test_double_extremes_aggregation_only(filled, bare, where):
    """+/-inf, +/-5e-324, +/-DBL_MAX, +/-FLT_MAX and the smallest float subnormal through MIN / MAX / SUM of raw DOUBLE,
    raw FLOAT and dictionary DOUBLE columns without GROUP BY: lane (raw and dictionary kernels), LDS and global."""
    for t in (filled, bare):
        for aggs, variant in (("SUM(rd), MIN(rd), MAX(rd), COUNT(*)", "lane_raw"), ("SUM(rf), MIN(rf), MAX(rf)", "lane_raw"),
                              ("SUM(dd), MIN(dd), MAX(dd)", "lane_dict")):
            run_case(t, aggs, where=where, plan={"strategy": "lane", "variant": variant})
            run_case(t, aggs, where=where, flags=L.PA_QF_NO_LANE_ACC | L.PA_QF_FORCE_LDS, plan={"strategy": "lds"})
            run_case(t, aggs, where=where, flags=L.PA_QF_NO_LANE_ACC | L.PA_QF_FORCE_GLOBAL, plan={"strategy": "global"})
