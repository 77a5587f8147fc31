"""Group trim: trim.py's order words against the host trim (reduce.server_trim), and the lowering with its refusals.
No GPU: the numpy restatement (trim.reference_trim) is what the device kernels implement word for word."""
import itertools
import random

import numpy as np
import pytest

from pinot_amd import _lib as L
from pinot_amd import trim as TR
from pinot_amd.engine import AvgPair, IntermediateResult, MinMaxRangePair
from pinot_amd.reduce import server_trim
from pinot_amd.query import parse_sql

AGGS = "COUNT(*), SUM(m), MIN(m), MAX(m), AVG(m), MINMAXRANGE(m)"
# the accumulators an executor plans for AGGS: COUNT, SUM(m), MIN(m), MAX(m); AVG shares the SUM, MINMAXRANGE (MIN, MAX)
AGG_MAP = [0, 1, 2, 3, 1, (2, 3)]
SPECIAL_SUMS = [0.0, -0.0, -1.0, 1.0, 2.0 ** 53, 2.0 ** 53 + 2, -(2.0 ** 53) - 2, 2.0 ** 60, -(2.0 ** 60), 9.007199254740993e15,
                1e300, -1e300, 0.5, -0.5]


def make_block(seed, cards, fill=0.6, equal_counts=False, strings=(1,)):
    """A random results block over len(cards) group-by columns (those in `strings` are STRING) with the arrays behind
    it: (the columns' sorted dictionaries, the block's groups, keys, counts, finals per accumulator of AGG_MAP)."""
    rng = random.Random(seed)
    dicts = []
    for j, c in enumerate(cards):
        if j in strings:
            dicts.append(sorted({"v%s%d" % ("x" * rng.randrange(3), i) for i in range(c * 2)})[:c])
        else:
            dicts.append(sorted(rng.sample(range(-1000, 1000), c)))
    K = int(np.prod(cards))
    keys = np.array(sorted(rng.sample(range(K), max(1, int(K * fill)))), dtype=np.int64)
    n = len(keys)
    counts = np.array([3 if equal_counts else rng.choice([1, 1, 2, 3, 7, 1000]) for _ in range(n)], dtype=np.int64)
    sums = np.array([rng.choice(SPECIAL_SUMS) if rng.random() < 0.5 else float(rng.randrange(-50, 50))
                     for _ in range(n)])
    mins = np.array([float(rng.randrange(-20, 20)) for _ in range(n)])
    maxs = mins + np.array([float(rng.randrange(0, 6)) for _ in range(n)])
    finals = [counts.astype(np.float64), sums, mins, maxs]
    groups = {}
    for i, k in enumerate(keys.tolist()):
        kv, rem = [], k
        for d in dicts:
            kv.append(d[rem % len(d)])
            rem //= len(d)
        groups[tuple(kv)] = [int(counts[i]), float(sums[i]), float(mins[i]), float(maxs[i]),
                             AvgPair(float(sums[i]), int(counts[i])), MinMaxRangePair(float(mins[i]), float(maxs[i]))]
    return dicts, groups, keys, counts, finals


def kept_by_host(sql, groups):
    q = parse_sql(sql)
    res = IntermediateResult(list(q.aggregations), list(q.group_by), dict(groups))
    return q, set(server_trim(res, q).groups)


def kept_by_words(q, dicts, keys, counts, finals):
    cards = [len(d) for d in dicts]
    terms = TR.lower_order_by(q, AGG_MAP)
    pos = TR.reference_trim(keys, cards, counts, finals, terms, TR.trim_size(q))
    out = set()
    for k in keys[pos].tolist():
        kv = []
        for d in dicts:
            kv.append(d[k % len(d)])
            k //= len(d)
        out.add(tuple(kv))
    return out


TERMS = ["g0", "g1", "COUNT(*)", "SUM(m)", "MIN(m)", "MAX(m)", "AVG(m)", "MINMAXRANGE(m)"]
ORDERS = ([[(t, d)] for t in TERMS for d in ("", " DESC")] +
          [[("COUNT(*)", " DESC"), ("SUM(m)", "")], [("AVG(m)", ""), ("g1", " DESC")],
           [("MINMAXRANGE(m)", " DESC"), ("MIN(m)", " DESC")], [("SUM(m)", " DESC"), ("COUNT(*)", "")],
           [("g1", " DESC"), ("SUM(m)", ""), ("AVG(m)", " DESC")], [("COUNT(*)", ""), ("MAX(m)", " DESC"), ("g0", " DESC")]])


@pytest.mark.parametrize("order", ORDERS, ids=lambda o: ",".join(t + d for t, d in o).replace(" ", "_"))
def test_words_keep_the_groups_the_host_trim_keeps(order):
    for seed, cards, strings in ((1, (7, 5), (1,)), (2, (4, 3, 6), (0, 2)), (3, (11, 9), ())):
        dicts, groups, keys, counts, finals = make_block(seed, cards, strings=strings)
        gb = ", ".join("g%d" % j for j in range(len(cards)))
        for limit in (1, 3, 9):
            sql = ("SELECT %s, %s FROM t GROUP BY %s ORDER BY %s LIMIT %d OPTION(minServerGroupTrimSize=1)"
                   % (gb, AGGS, gb, ", ".join(t + d for t, d in order), limit))
            q, want = kept_by_host(sql, groups)
            assert len(want) == min(len(groups), 5 * limit)
            assert kept_by_words(q, dicts, keys, counts, finals) == want, sql


def test_no_order_by_keeps_the_lowest_key_tuples():
    dicts, groups, keys, counts, finals = make_block(5, (6, 4, 3), strings=(1,))
    sql = "SELECT g0, g1, g2, %s FROM t GROUP BY g0, g1, g2 LIMIT 7" % AGGS
    q, want = kept_by_host(sql, groups)
    assert len(want) == 7 and want == set(sorted(groups)[:7])
    assert TR.lower_order_by(q, AGG_MAP) == [] and TR.trim_size(q) == 7
    assert kept_by_words(q, dicts, keys, counts, finals) == want


@pytest.mark.parametrize("desc", ["", " DESC"])
def test_heavy_ties_cut_inside_a_tie_class(desc):
    """Every count equal: the kept groups are decided by the tie word alone (key tuples ascending, also under DESC)."""
    dicts, groups, keys, counts, finals = make_block(7, (9, 8), equal_counts=True)
    sql = ("SELECT g0, g1, %s FROM t GROUP BY g0, g1 ORDER BY COUNT(*)%s LIMIT 2 OPTION(minServerGroupTrimSize=1)"
           % (AGGS, desc))
    q, want = kept_by_host(sql, groups)
    assert want == set(sorted(groups)[:10])
    assert kept_by_words(q, dicts, keys, counts, finals) == want


def test_fewer_groups_than_the_trim_keeps_all():
    dicts, groups, keys, counts, finals = make_block(9, (3, 2))
    sql = "SELECT g0, g1, %s FROM t GROUP BY g0, g1 ORDER BY SUM(m) LIMIT 10" % AGGS
    q, want = kept_by_host(sql, groups)
    assert want == set(groups) and kept_by_words(q, dicts, keys, counts, finals) == want


def test_double_words_order_like_the_host_compares():
    vals = np.array([-np.inf, -1e300, -2.0 ** 53 - 2, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 2.0 ** 53, 2.0 ** 53 + 2, 1e300,
                     np.inf])
    w = TR.double_word(vals)
    for a, b in itertools.combinations(range(len(vals)), 2):
        assert (w[a] < w[b]) == (vals[a] < vals[b]) and (w[a] == w[b]) == (vals[a] == vals[b]), (vals[a], vals[b])
    assert w[5] == w[6]  # -0.0 ties with +0.0


def test_lowering():
    q = parse_sql("SELECT g0, g1, %s FROM t GROUP BY g0, g1 ORDER BY g1 DESC, COUNT(*), SUM(m) DESC, MINMAXRANGE(m) "
                  "LIMIT 4" % AGGS)
    assert TR.lower_order_by(q, AGG_MAP) == [(L.PA_TRIM_KEY_COLUMN, 1, 0, 1), (L.PA_TRIM_COUNT, 0, 0, 0),
                                             (L.PA_TRIM_AGG, 1, 0, 1), (L.PA_TRIM_RANGE, 3, 2, 0)]
    assert TR.trim_size(q) == 5000  # max(5 * limit, minServerGroupTrimSize's default)
    q = parse_sql("SELECT g0, AVG(m), MAX(m) FROM t GROUP BY g0 ORDER BY AVG(m), MAX(m) DESC LIMIT 2000")
    assert TR.lower_order_by(q, [0, 1]) == [(L.PA_TRIM_AVG, 0, 0, 0), (L.PA_TRIM_AGG, 1, 0, 1)]
    assert TR.trim_size(q) == 10000
    spec = TR.build_spec(TR.lower_order_by(q, [0, 1]), TR.trim_size(q))
    assert (spec.num_terms, list(spec.kind)[:2], list(spec.index)[:2], list(spec.desc)[:2], spec.trim) == (
        2, [L.PA_TRIM_AVG, L.PA_TRIM_AGG], [0, 1], [0, 1], 10000)


REFUSED = [
    ("SELECT g0, DISTINCTCOUNT(m) FROM t GROUP BY g0 ORDER BY DISTINCTCOUNT(m) LIMIT 3", [0]),
    ("SELECT g0, DISTINCTCOUNTHLL(m) FROM t GROUP BY g0 ORDER BY DISTINCTCOUNTHLL(m) LIMIT 3", [0]),
    ("SELECT g0, DISTINCTCOUNTRAWHLL(m) FROM t GROUP BY g0 ORDER BY DISTINCTCOUNTRAWHLL(m) LIMIT 3", [0]),
    ("SELECT g0, PERCENTILE50(m) FROM t GROUP BY g0 ORDER BY PERCENTILE50(m) LIMIT 3", [0]),
    ("SELECT g0, COUNT(*), PERCENTILE50(m) FROM t GROUP BY g0 ORDER BY COUNT(*) LIMIT 3", [0, 1]),  # (only selected)
    ("SELECT g0, DISTINCTSUM(m) FROM t GROUP BY g0 ORDER BY DISTINCTSUM(m) LIMIT 3", [0]),
    ("SELECT g0, DISTINCTAVG(m) FROM t GROUP BY g0 ORDER BY DISTINCTAVG(m) LIMIT 3", [0]),
    ("SELECT g0, COUNTMV(v) FROM t GROUP BY g0 ORDER BY COUNTMV(v) LIMIT 3", [0]),
    ("SELECT g0, AVGMV(v) FROM t GROUP BY g0 ORDER BY AVGMV(v) LIMIT 3", [(0, 1)]),
    ("SELECT g0, SUM(m) FILTER (WHERE x > 3) FROM t GROUP BY g0 ORDER BY SUM(m) FILTER (WHERE x > 3) LIMIT 3", [0]),
    ("SELECT g0, COUNT(*), SUM(m) FILTER (WHERE x > 3) FROM t GROUP BY g0 ORDER BY COUNT(*) LIMIT 3", [0, 1]),
    ("SELECT g0, COUNT(*) FROM t GROUP BY g0, g1, g2, g3, g4 ORDER BY g0, g1, g2, g3, g4 LIMIT 3", [0]),
    ("SELECT ADD(g0, 1), COUNT(*) FROM t GROUP BY ADD(g0, 1) ORDER BY COUNT(*) LIMIT 3", [0]),
]


@pytest.mark.parametrize("sql,agg_map", REFUSED, ids=[r[0][7:60].replace(" ", "_") for r in REFUSED])
def test_refused_shapes_trim_on_the_host(sql, agg_map):
    with pytest.raises(TR.HostTrim):
        TR.lower_order_by(parse_sql(sql), agg_map)


def test_hashed_key_space_is_refused_and_selected_sketches_are_not():
    q = parse_sql("SELECT g0, COUNT(*) FROM t GROUP BY g0 ORDER BY COUNT(*) LIMIT 3")
    with pytest.raises(TR.HostTrim):
        TR.lower_order_by(q, [0], hashed=True)
    q = parse_sql("SELECT g0, SUM(m), DISTINCTCOUNTHLL(m), DISTINCTCOUNT(m) FROM t GROUP BY g0 ORDER BY SUM(m) DESC LIMIT 3")
    assert TR.lower_order_by(q, [0, 1, 2]) == [(L.PA_TRIM_AGG, 0, 0, 1)]
