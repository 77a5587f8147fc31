"""Two independent references for queries with filtered aggregations (AGG(x) FILTER (WHERE f)), the checkers of
tests/test_filtered.py and tests/test_gpu_filtered.py. They use the product only for parse_sql's Query model, the
Segment model and the intermediate value classes.

(a) compose: the reference's own test method (FilteredAggregationsTest.java: a filtered column equals the unfiltered
    query with the filter moved into WHERE) — one oracle.run_query per swim lane with filter `W AND F_j`, the groups
    united, a lane's aggregations at their empty values in the groups it did not see
    (FilteredGroupByOperator.java:117-150), the statistics summed per segment over that segment's lanes
    (AggregationFunctionUtils.java:312-396, FilteredAggregationOperator.java:96-98).
(b) numpy_eval: masks on the decoded columns, np.unique keys, Python-int sums.
"""
import dataclasses

import numpy as np

import oracle
import selection_ref as SR
from pinot_amd import query as Q
from pinot_amd.engine import AvgPair, IntermediateResult, MinMaxRangePair
from pinot_amd.hll import HyperLogLog


def lane_filters(query):
    """The distinct FILTER clauses, as written, in first-use order."""
    out = []
    for a in query.aggregations:
        if a.filter is not None and a.filter not in out:
            out.append(a.filter)
    return out


def empty_value(a):
    fn = Q.base_function(a.function)
    if fn == "COUNT":
        return 0
    if fn == "SUM":
        return 0.0
    if fn == "MIN":
        return float("inf")
    if fn == "MAX":
        return float("-inf")
    if fn == "AVG":
        return AvgPair(0.0, 0)
    if fn == "MINMAXRANGE":
        return MinMaxRangePair(float("inf"), float("-inf"))
    if fn in ("DISTINCTCOUNTHLL", "DISTINCTCOUNTRAWHLL"):
        return HyperLogLog(a.log2m)
    return set()


def _and(w, f):
    if w is None:
        return f
    return Q.And((w, f))


def lane_query(query, f, aggs):
    """The unfiltered query of one lane: its aggregations without their FILTER, the lane's filter moved into WHERE."""
    plain = [dataclasses.replace(a, filter=None) for a in aggs]
    return dataclasses.replace(query, aggregations=plain, aliases=[None] * len(plain),
                               filter=query.filter if f is None else _and(query.filter, f), order_by=[],
                               num_select_aggs=len(plain))


# ------------------------------------------------------------------ the per-segment lane rule
def dictionary_constant(f, seg):
    """"all" / "empty" when the filter's predicates are constant over the segment's dictionaries: a predicate on a
    dictionary column matching every dictionary value is always true, one matching none always false (the dictionary
    based predicate evaluators); AND / OR / NOT fold them (FilterOperatorUtils). Evaluated on a one-doc-per-value
    view of each dictionary, so it shares no code with the product's constant folding."""
    if f is None:
        return "all"
    if isinstance(f, Q.BoolFilter):
        return "all" if f.value else "empty"
    if isinstance(f, (Q.And, Q.Or)):
        ks = [dictionary_constant(c, seg) for c in f.children]
        whole, unit = ("empty", "all") if isinstance(f, Q.And) else ("all", "empty")
        if whole in ks:
            return whole
        return unit if all(k == unit for k in ks) else None
    if isinstance(f, Q.Not):
        return {"all": "empty", "empty": "all"}.get(dictionary_constant(f.child, seg))
    col = seg.column(f.column)
    if not col.has_dictionary:
        return None
    view = _DictView(seg, f.column)
    m = SR.filter_mask(f, view)
    return "all" if m.all() else ("empty" if not m.any() else None)


class _DictView:
    """A segment-like whose one column holds every dictionary value once."""

    def __init__(self, seg, name):
        self.col = seg.column(name)
        self.name = name
        self.num_docs = len(self.col.dictionary)

    def column(self, name):
        assert name == self.name
        d = np.asarray(self.col.dictionary)

        class C:
            data_type = self.col.data_type
            has_dictionary = False
            raw_values = d
        return C


def segment_lanes(query, seg):
    """[(filter or None, aggregations)]: the swim lanes of one segment (None: the main lane)."""
    main = dictionary_constant(query.filter, seg)
    if main == "empty":
        return []  # one lane whose filter matches nothing: no doc, no entry
    lanes = []
    main_aggs = [a for a in query.aggregations if a.filter is None]
    for f in lane_filters(query):
        aggs = [a for a in query.aggregations if a.filter == f]
        if main != "all" and dictionary_constant(f, seg) == "all":
            main_aggs += aggs  # the sub filter's operator is match-all: the lane runs on the main filter's operator
        else:
            lanes.append((f, aggs))
    if main_aggs:
        lanes.append((None, main_aggs))
    return lanes


def projected(query, aggs):
    cols = list(query.group_by)
    for a in aggs:
        if a.column is not None and a.column not in cols:
            cols.append(a.column)
    return len(cols)


def statistics(query, segments, docs_of):
    """(numDocsScanned, numEntriesScannedPostFilter): docs_of(segment, filter tree or None) -> docs matching it."""
    scanned = post = 0
    for seg in segments:
        if seg.num_docs == 0:
            continue
        for f, aggs in segment_lanes(query, seg):
            n = docs_of(seg, query.filter if f is None else _and(query.filter, f))
            scanned += n
            post += n * projected(query, aggs)
    return scanned, post


# ------------------------------------------------------------------ (a) the composition over the oracle
def compose(query, segments):
    segments = list(segments)
    res = IntermediateResult(list(query.aggregations), list(query.group_by))
    res.num_total_docs = sum(s.num_docs for s in segments)
    live = [s for s in segments if s.num_docs > 0]
    per_lane = {}
    for f in [None] + lane_filters(query):
        idx = [i for i, a in enumerate(query.aggregations) if a.filter == f]
        if not idx:
            continue
        r = oracle.run_query(lane_query(query, f, [query.aggregations[i] for i in idx]), live) if live else None
        per_lane[f] = (idx, r)
    if query.group_by:
        keys = []
        for idx, r in per_lane.values():
            for k in (r.groups if r is not None else {}):
                if k not in keys:
                    keys.append(k)
        for k in keys:
            row = [empty_value(a) for a in query.aggregations]
            for idx, r in per_lane.values():
                if k in r.groups:
                    for i, v in zip(idx, r.groups[k]):
                        row[i] = v
            res.groups[k] = row
    else:
        row = [empty_value(a) for a in query.aggregations]
        for idx, r in per_lane.values():
            if r is not None:
                for i, v in zip(idx, r.row):
                    row[i] = v
        res.row = row

    def docs_of(seg, filt):
        q1 = dataclasses.replace(Q.parse_sql("SELECT COUNT(*) FROM t"), filter=filt)
        return oracle.run_query(q1, [seg]).num_docs_scanned
    res.num_docs_scanned, res.num_entries_scanned_post_filter = statistics(query, live, docs_of)
    res.num_entries_scanned_in_filter = None
    return res


# ------------------------------------------------------------------ (b) numpy on the decoded columns
def _agg_numpy(a, values, dt):
    fn = a.function
    n = len(values)
    if fn == "COUNT":
        return n
    if fn in ("SUM", "AVG"):
        if dt in ("INT", "LONG"):
            s = float(sum(int(v) for v in values.tolist()))  # exact, rounded once
        else:
            s = float(np.sum(values.astype(np.float64))) if n else 0.0
        return s if fn == "SUM" else AvgPair(s, n)
    if fn == "MIN":
        return float(values.min()) if n else float("inf")
    if fn == "MAX":
        return float(values.max()) if n else float("-inf")
    if fn == "MINMAXRANGE":
        return MinMaxRangePair(float(values.min()), float(values.max())) if n else empty_value(a)
    if fn in ("DISTINCTCOUNTHLL", "DISTINCTCOUNTRAWHLL"):
        h = HyperLogLog(a.log2m)
        for v in np.unique(values).tolist():
            h.offer(v, dt)
        return h
    if fn == "DISTINCTCOUNT":
        return set(np.unique(values).tolist())
    raise NotImplementedError(fn)


def numpy_eval(query, segments):
    segments = [s for s in segments]
    res = IntermediateResult(list(query.aggregations), list(query.group_by))
    res.num_total_docs = sum(s.num_docs for s in segments)
    live = [s for s in segments if s.num_docs > 0]
    cols = {}

    def column(name):
        if name not in cols:
            cols[name] = np.concatenate([SR.decoded(s, name) for s in live]) if live else np.zeros(0)
        return cols[name]
    w = np.concatenate([SR.filter_mask(query.filter, s) for s in live]) if live else np.zeros(0, bool)
    masks = []
    for a in query.aggregations:
        m = w if a.filter is None else (w & np.concatenate([SR.filter_mask(a.filter, s) for s in live]))
        masks.append(m)
    union = np.zeros(len(w), bool)
    for m in masks:
        union |= m
    dts = {a.column: live[0].column(a.column).data_type for a in query.aggregations if a.column} if live else {}
    if query.group_by:
        gcols = [column(c) for c in query.group_by]
        rows = np.flatnonzero(union)
        seen = {}
        for r in rows.tolist():
            seen.setdefault(tuple(g[r].item() for g in gcols), []).append(r)
        for k, docs in seen.items():
            docs = np.asarray(docs)
            vals = []
            for a, m in zip(query.aggregations, masks):
                sel = docs[m[docs]]
                v = column(a.column)[sel] if a.column else sel
                vals.append(_agg_numpy(a, v, dts.get(a.column)))
            res.groups[k] = vals
    else:
        vals = []
        for a, m in zip(query.aggregations, masks):
            sel = np.flatnonzero(m)
            v = column(a.column)[sel] if a.column else sel
            vals.append(_agg_numpy(a, v, dts.get(a.column)))
        res.row = vals

    def docs_of(seg, filt):
        return int(SR.filter_mask(filt, seg).sum())
    res.num_docs_scanned, res.num_entries_scanned_post_filter = statistics(query, live, docs_of)
    res.num_entries_scanned_in_filter = None
    return res


# ------------------------------------------------------------------ comparison
def _same_value(fn, a, b, double_sum_rtol):
    fn = Q.base_function(fn)
    if fn in ("DISTINCTCOUNTHLL", "DISTINCTCOUNTRAWHLL"):
        return np.array_equal(np.asarray(a.registers), np.asarray(b.registers))
    if fn == "AVG":
        return a.count == b.count and _same_value("SUM", a.sum, b.sum, double_sum_rtol)
    if fn == "MINMAXRANGE":
        return (a.min, a.max) == (b.min, b.max)
    if fn == "SUM" and double_sum_rtol:
        return abs(a - b) <= double_sum_rtol * max(abs(a), abs(b))
    if fn in ("DISTINCTCOUNT", "DISTINCTSUM", "DISTINCTAVG"):
        return set(a) == set(b)
    return a == b


def assert_same(got, ref, double_sum_columns=(), rtol=1e-9, stats=True, totals=True):
    """Exact equality of the groups / the row (DOUBLE sums of `double_sum_columns` within rtol) and of numDocsScanned,
    numEntriesScannedPostFilter, numTotalDocs; numEntriesScannedInFilter is None on both sides. stats / totals = False
    leave the statistics / numTotalDocs out (one rank's merged block: they are that rank's own)."""
    aggs = ref.aggregations

    def rt(a):
        return rtol if a.column in double_sum_columns else 0.0
    if ref.group_by:
        assert set(got.groups) == set(ref.groups), (sorted(set(got.groups) ^ set(ref.groups))[:5],)
        for k, row in ref.groups.items():
            for a, x, y in zip(aggs, got.groups[k], row):
                assert _same_value(a.function, x, y, rt(a)), (k, a.result_name, x, y)
    else:
        for a, x, y in zip(aggs, got.row, ref.row):
            assert _same_value(a.function, x, y, rt(a)), (a.result_name, x, y)
    if totals:
        assert got.num_total_docs == ref.num_total_docs
    if stats:
        assert got.num_docs_scanned == ref.num_docs_scanned
        assert got.num_entries_scanned_post_filter == ref.num_entries_scanned_post_filter
        assert got.num_entries_scanned_in_filter is None and ref.num_entries_scanned_in_filter is None
