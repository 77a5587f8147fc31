"""Reference for transform-expression queries (SUM(ADD(a, b)), GROUP BY timeConvert(...)): every expression is evaluated on
the host (pinot_amd.transform.evaluate, the numpy restatement of the device program), added to a copy of each segment
as a materialised raw column (DOUBLE or LONG), and the same query over those plain columns runs through the unmodified
oracle, which groups raw columns by value and sums raw LONG values exactly.

Equality: exact for group keys (compared as bits: every NaN one key, -0.0 and 0.0 two), counts, MIN, MAX, LONG sums, and
DOUBLE sums over integer-valued data (exact=True). Other DOUBLE sums: the project's relative 1e-9
(tests/test_gpu_parity.py), taken against the sum of the values' magnitudes in the group — the reference query carries
one more SUM over the materialised |value| column for it — so a SUB's cancellation cannot make the bound vacuous."""
import dataclasses
import struct

import numpy as np

import oracle
from pinot_amd import query as Q
from pinot_amd import transform as T
from pinot_amd.engine import AvgPair, MinMaxRangePair
from pinot_amd.segment import Segment, build_column, unpack_bits

REL = 1e-9


def column_values(seg, name):
    c = seg.column(name)
    if not c.has_dictionary:
        return np.asarray(c.raw_values)
    return np.asarray(c.dictionary)[unpack_bits(c.fwd_bytes, seg.num_docs, c.num_bits)]


def expressions_of(query):
    out = []
    for item in list(query.group_by) + [a.column for a in query.aggregations]:
        if isinstance(item, Q.Expr) and item not in out:
            out.append(item)
    return out


def expr_values(expr, seg):
    return T.evaluate(expr, {c: column_values(seg, c) for c in expr.columns()})


def materialise(query, segs):
    """(query over plain columns, segments with the materialised columns, index of the magnitude SUM of every
    aggregation or None). Expression e becomes the raw column __e<i>, its magnitudes __m<i>."""
    exprs = expressions_of(query)
    name = {e: "__e%d" % i for i, e in enumerate(exprs)}
    out_segs = []
    for s in segs:
        m = Segment(name=s.name, num_docs=s.num_docs, columns=dict(s.columns))
        for i, e in enumerate(exprs):
            v = expr_values(e, s)
            dt = "DOUBLE" if v.dtype.kind == "f" else "LONG"
            m.columns["__e%d" % i] = build_column("__e%d" % i, v, dt, has_dictionary=False)
            if dt == "DOUBLE":
                m.columns["__m%d" % i] = build_column("__m%d" % i, np.abs(np.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0)),
                                                      "DOUBLE", has_dictionary=False)
        out_segs.append(m)
    aggs = [dataclasses.replace(a, column=name.get(a.column, a.column)) if isinstance(a.column, Q.Expr) else a
            for a in query.aggregations]
    mags = []
    for a in query.aggregations:
        if isinstance(a.column, Q.Expr) and a.function in ("SUM", "AVG") and T.infer_type(a.column) == T.DOUBLE:
            aggs.append(Q.Aggregation("SUM", "__m%d" % exprs.index(a.column)))
            mags.append(len(aggs) - 1)
        else:
            mags.append(None)
    mq = dataclasses.replace(query, aggregations=aggs, aliases=[None] * len(aggs),
                             group_by=[name.get(g, g) if isinstance(g, Q.Expr) else g for g in query.group_by],
                             order_by=[], select_columns=[])
    return mq, out_segs, mags


def reference(query, segs):
    mq, msegs, mags = materialise(query, segs)
    return oracle.run_query(mq, msegs), mags


def key_bits(k):
    """A group key as comparable bits per component (doubles by doubleToLongBits)."""
    out = []
    for v in k:
        if isinstance(v, (float, np.floating)):
            v = float(v)
            out.append(("d", 0x7ff8000000000000 if v != v else struct.unpack("<Q", struct.pack("<d", v))[0]))
        elif isinstance(v, (int, np.integer)):
            out.append(("i", int(v)))
        else:
            out.append(("s", v))
    return tuple(out)


def _close(got, want, mag, exact):
    if exact or mag is None:
        return got == want or (got != got and want != want)
    return abs(got - want) <= REL * mag or got == want


def assert_same(got, ref, query, mags, exact=True):
    """got: the GPU's IntermediateResult of `query`; ref: the oracle's of the materialised query."""
    assert got.num_docs_scanned == ref.num_docs_scanned
    assert got.num_total_docs == ref.num_total_docs
    ncols = len(query.aggregations)
    if query.group_by:
        g = {key_bits(k): (k, v) for k, v in got.groups.items()}
        r = {key_bits(k): v for k, v in ref.groups.items()}
        assert len(g) == len(got.groups), "GPU group keys collide as bits"
        assert set(g) == set(r), (sorted(set(g) ^ set(r))[:5], len(g), len(r))
        for j, item in enumerate(query.group_by):  # key types: LONG as ints, DOUBLE as floats
            if isinstance(item, Q.Expr):
                want = float if T.infer_type(item) == T.DOUBLE else int
                assert all(isinstance(k[j], want) and not isinstance(k[j], bool) for k, _ in g.values()), (item, want)
        rows = [(kb, g[kb][1], r[kb]) for kb in g]
    else:
        rows = [((), got.row, ref.row)]
    for kb, gv, rv in rows:
        for i, a in enumerate(query.aggregations[:ncols]):
            x, y = gv[i], rv[i]
            mag = rv[mags[i]] if mags[i] is not None else None
            if isinstance(y, AvgPair):
                assert x.count == y.count, (kb, a)
                assert _close(x.sum, y.sum, mag, exact), (kb, a.result_name, x.sum, y.sum, mag)
            elif isinstance(y, MinMaxRangePair):
                assert (x.min, x.max) == (y.min, y.max), (kb, a.result_name, x, y)
            elif isinstance(y, float) or isinstance(x, float):
                assert _close(x, y, mag if a.function == "SUM" else None, exact or a.function != "SUM"), \
                    (kb, a.result_name, x, y, mag)
            else:
                assert x == y, (kb, a.result_name, x, y)


def post_filter_entries(query, docs_scanned):
    """numDocsScanned x the distinct columns the group-by items and aggregation arguments read
    (AggregationOperator.java:86, GroupByOperator.java:146)."""
    cols = []
    for item in list(query.group_by) + [a.column for a in query.aggregations]:
        Q.item_columns(item, cols)
    return docs_scanned * len(cols)


def sums_are_exact(values):
    """Every value is a finite multiple of 2^-k (some k <= 4) and their magnitudes sum below 2^(53 - k): every partial
    sum, in any order, is a multiple of 2^-k below 2^(53 - k), hence a double, so a DOUBLE sum over them is exact
    whatever the atomics' order."""
    v = np.asarray(values, dtype=np.float64)
    if not len(v):
        return True
    if not np.all(np.isfinite(v)):
        return False
    for k in range(5):
        if np.all(v * 2.0 ** k == np.floor(v * 2.0 ** k)):
            return bool(np.abs(v).sum() * 2.0 ** k < 2.0 ** 53)
    return False


def double_sums_exact(query, segs):
    """exact=True is justified: the values of every DOUBLE expression (and FLOAT / DOUBLE column) under SUM / AVG, over
    all docs of all segments together, pass sums_are_exact."""
    for a in query.aggregations:
        if a.function not in ("SUM", "AVG") or a.column is None:
            continue
        if isinstance(a.column, Q.Expr):
            if T.infer_type(a.column) != T.DOUBLE:
                continue
            v = np.concatenate([expr_values(a.column, s) for s in segs])
        else:
            if segs[0].column(a.column).data_type not in ("FLOAT", "DOUBLE"):
                continue
            v = np.concatenate([column_values(s, a.column) for s in segs])
        if not sums_are_exact(v):
            return False
    return True

