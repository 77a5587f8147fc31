"""Server trim + broker reduce of intermediate results (the callers either side of the hot path).

  merge_intermediate   ~ GroupByDataTableReducer / AggregationDataTableReducer merging server DataTables
                         (AggregationFunction.merge: COUNT/SUM +, MIN min, MAX max, AVG pair +, HLL addAll,
                         MINMAXRANGE pair min/max, DISTINCTCOUNT / DISTINCTSUM / DISTINCTAVG set union,
                         PERCENTILE addAll = value histogram counts added,
                         FIRSTWITHTIME / LASTWITHTIME the pair of the earlier / later time, the first argument on a tie,
                         VARPOP / VARSAMP / STDDEVPOP / STDDEVSAMP VarianceTuple.apply, COVARPOP / COVARSAMP
                         CovarianceTuple.apply)
  server_trim          ~ IndexedTable.finish on the server (IndexedTable.java:149): with ORDER BY keep the top
                         max(limit*5, minServerGroupTrimSize) groups (GroupByUtils.getTableCapacity); without
                         ORDER BY keep `limit` groups (GroupByCombineOperator.java:63-73)
  final_result_table   ~ broker: extractFinalResult (AVG sum/count, HLL cardinality), ORDER BY, LIMIT
  merge_selection      ~ broker: SelectionOperatorService.reduceWithOrdering / SelectionDataTableReducer (the servers'
                         sorted rows merged under the ORDER BY comparator, `offset` rows dropped, `limit` kept,
                         projected to the select list)
"""
import math
from functools import cmp_to_key

from . import query as Q
from .engine import AvgPair, CovarianceTuple, IntermediateResult, MinMaxRangePair, VarianceTuple
from .hll import HyperLogLog


def merge_value(fn, a, b):
    fn = Q.base_function(fn)
    if fn in ("COUNT", "SUM"):
        return a + b
    if fn == "MIN":
        return min(a, b)
    if fn == "MAX":
        return max(a, b)
    if fn == "AVG":
        return AvgPair(a.sum + b.sum, a.count + b.count)
    if fn in ("DISTINCTCOUNTHLL", "DISTINCTCOUNTRAWHLL"):
        return HyperLogLog(a.log2m, a.registers).add_all(b)
    if fn == "MINMAXRANGE":  # MinMaxRangePair.apply
        return MinMaxRangePair(min(a.min, b.min), max(a.max, b.max))
    if fn in ("DISTINCTCOUNT", "DISTINCTSUM", "DISTINCTAVG", "DISTINCTCOUNTBITMAP"):
        # BaseDistinctAggregateAggregationFunction.merge: union (DISTINCTCOUNTBITMAP: RoaringBitmap.or)
        return set(a) | set(b)
    if fn == "PERCENTILE":  # PercentileAggregationFunction.merge: DoubleArrayList.addAll (counts add per value)
        return a.merge(b)
    if fn == "LASTWITHTIME":  # LastWithTimeAggregationFunction.merge (:223): the first argument wins equal times
        return a if a.time >= b.time else b
    if fn == "FIRSTWITHTIME":  # FirstWithTimeAggregationFunction.merge (:227)
        return a if a.time <= b.time else b
    if fn in Q.VARIANCE_FUNCTIONS:
        # VarianceTuple.apply(VarianceTuple) (:46-55), in its order of operations: Chan et al.'s pairwise update
        if b.count == 0:
            return a
        curr_avg = 0.0 if a.count == 0 else a.sum / a.count
        delta = (b.sum / b.count) - curr_avg
        m2 = a.m2 + (b.m2 + delta * delta * b.count * a.count / (b.count + a.count))
        return VarianceTuple(a.count + b.count, a.sum + b.sum, m2)
    if fn in Q.COVARIANCE_FUNCTIONS:  # CovarianceTuple.apply(CovarianceTuple) (:51-56)
        return CovarianceTuple(a.sum_x + b.sum_x, a.sum_y + b.sum_y, a.sum_xy + b.sum_xy, a.count + b.count)
    raise ValueError(fn)


def final_value(fn, v):
    """extractFinalResult. fn: the function's name, or the Aggregation (PERCENTILE needs its percentile)."""
    agg = fn if isinstance(fn, Q.Aggregation) else None
    fn = Q.base_function(agg.function if agg is not None else fn)
    if fn == "PERCENTILE":
        # PercentileAggregationFunction.extractFinalResult: -inf (DEFAULT_FINAL_RESULT) for an empty list, else the
        # sorted values' element at the percentile's rank (engine.ValueHistogram.value_at)
        if agg is None:
            raise ValueError("PERCENTILE's final value needs the Aggregation (its percentile), not the name")
        return v.value_at(agg.percentile)
    if fn == "AVG":
        return v.sum / v.count if v.count else -math.inf
    if fn == "DISTINCTCOUNTHLL":
        return v.cardinality()
    if fn == "DISTINCTCOUNTRAWHLL":
        return SerializedHLL(v)
    if fn == "MINMAXRANGE":  # MinMaxRangeAggregationFunction.extractFinalResult: max - min
        return v.max - v.min
    if fn in ("DISTINCTCOUNT", "DISTINCTCOUNTBITMAP"):  # extractFinalResult: the set's size / the bitmap's cardinality
        return len(v)
    if fn in ("DISTINCTSUM", "DISTINCTAVG"):
        # DistinctSumAggregationFunction / DistinctAvgAggregationFunction.extractFinalResult: a double sum over the set
        # in its iteration order, divided by its size for the average (0/0 = NaN for an empty set, as in Java). The
        # reference iterates a Java HashSet, this a Python set: for non-integer FLOAT/DOUBLE values the sums can differ
        # in the last bits (parity unpinned: no golden vector sums fractional distinct values; tests compare those
        # with a relative tolerance)
        s = 0.0
        for x in v:
            s += float(x)
        if fn == "DISTINCTSUM":
            return s
        return s / len(v) if len(v) else math.nan
    if fn in Q.VARIANCE_FUNCTIONS:
        # VarianceAggregationFunction.extractFinalResult (:228-248): DEFAULT_FINAL_RESULT = -inf for no doc, and for one
        # doc under the sample forms
        n = v.count
        sample = fn in ("VARSAMP", "STDDEVSAMP")
        if n == 0 or (sample and n - 1 == 0):
            return -math.inf
        var = v.m2 / (n - 1) if sample else v.m2 / n
        if fn in ("STDDEVPOP", "STDDEVSAMP"):
            return math.sqrt(var) if var >= 0 else math.nan  # (Math.sqrt: NaN for NaN and negatives)
        return var
    if fn in Q.COVARIANCE_FUNCTIONS:
        # CovarianceAggregationFunction.extractFinalResult (:186-203); count * count is a long product in Java
        n = v.count
        if n == 0:
            return -math.inf
        if fn == "COVARSAMP":
            if n - 1 == 0:
                return -math.inf
            return (v.sum_xy / (n - 1)) - (v.sum_x * v.sum_y) / _java_long(n * (n - 1))
        return (v.sum_xy / n) - (v.sum_x * v.sum_y) / _java_long(n * n)
    if fn in Q.WITH_TIME_FUNCTIONS:
        # extractFinalResult: the pair's value; a 'BOOLEAN' pair holds the int (IntLongPair), the BOOLEAN result column
        # shows value != 0
        if agg is not None and agg.data_type == "BOOLEAN":
            return v.value != 0
        return v.value
    return v


def _java_long(x):
    """A Java long product: wraps at 64 bits."""
    return ((int(x) + (1 << 63)) & ((1 << 64) - 1)) - (1 << 63)


def _add_stat(a, b):
    return None if a is None or b is None else a + b


def merge_intermediate(results):
    results = list(results)
    out = IntermediateResult(results[0].aggregations, results[0].group_by)
    fns = [a.function for a in out.aggregations]
    for r in results:
        # (a statistic a server cannot define — numEntriesScannedInFilter of a query with filtered aggregations —
        # is None, and stays None in the sum)
        out.num_docs_scanned = _add_stat(out.num_docs_scanned, r.num_docs_scanned)
        out.num_total_docs += r.num_total_docs
        out.num_entries_scanned_in_filter = _add_stat(out.num_entries_scanned_in_filter, r.num_entries_scanned_in_filter)
        out.num_entries_scanned_post_filter = _add_stat(out.num_entries_scanned_post_filter,
                                                        r.num_entries_scanned_post_filter)
        out.num_groups_limit_reached |= r.num_groups_limit_reached
        if out.group_by:
            for k, vals in r.groups.items():
                if k in out.groups:
                    out.groups[k] = [merge_value(f, a, b) for f, a, b in zip(fns, out.groups[k], vals)]
                else:
                    out.groups[k] = list(vals)
        elif out.row is None:
            out.row = list(r.row)
        else:
            out.row = [merge_value(f, a, b) for f, a, b in zip(fns, out.row, r.row)]
    return out


class SerializedHLL(str):
    """DISTINCTCOUNTRAWHLL's final result (SerializedHLL.java): the string is BytesUtils.toHexString of
    HyperLogLog.getBytes(); ORDER BY compares cardinalities (compareTo)."""

    def __new__(cls, hll):
        s = str.__new__(cls, hll.to_bytes().hex())
        s.cardinality = hll.cardinality()
        return s


def _sort_value(v):
    return v.cardinality if isinstance(v, SerializedHLL) else v


def _order_key_fn(query):
    """Comparator over (key, final values) following ORDER BY; ties broken by group key for determinism."""
    items = []
    for ob in query.order_by:
        if isinstance(ob.expr, Q.Aggregation):
            idx = None
            for i, a in enumerate(query.aggregations):
                if a == ob.expr:
                    idx = i
            if idx is None:
                raise ValueError("ORDER BY aggregation not in select list: %r" % (ob.expr,))
            items.append(("agg", idx, ob.asc))
        else:
            items.append(("key", query.group_by.index(ob.expr), ob.asc))

    def cmp(x, y):
        for kind, idx, asc in items:
            a = _sort_value(x[1][idx]) if kind == "agg" else x[0][idx]
            b = _sort_value(y[1][idx]) if kind == "agg" else y[0][idx]
            if a != b:
                c = -1 if a < b else 1
                return c if asc else -c
        return -1 if x[0] < y[0] else (1 if x[0] > y[0] else 0)
    return cmp_to_key(cmp)


def server_trim(res: IntermediateResult, query: Q.Query) -> IntermediateResult:
    if not query.group_by:
        return res
    fns = list(query.aggregations)
    if query.order_by:
        trim = max(query.limit * 5, query.min_server_group_trim_size)
    else:
        trim = query.limit
    if len(res.groups) <= trim:
        return res
    rows = [(k, [final_value(f, v) for f, v in zip(fns, vals)], k) for k, vals in res.groups.items()]
    if query.order_by:
        rows.sort(key=_order_key_fn(query))
    else:
        rows.sort(key=lambda r: r[0])
    keep = {r[2] for r in rows[:trim]}
    out = IntermediateResult(res.aggregations, res.group_by, {k: v for k, v in res.groups.items() if k in keep})
    out.num_docs_scanned, out.num_total_docs = res.num_docs_scanned, res.num_total_docs
    out.num_entries_scanned_in_filter = res.num_entries_scanned_in_filter
    out.num_entries_scanned_post_filter = res.num_entries_scanned_post_filter
    out.num_groups_limit_reached = res.num_groups_limit_reached
    return out


def final_result_table(res: IntermediateResult, query: Q.Query):
    """Broker ResultTable rows: [select group-by columns..., final aggregation values...]."""
    fns = list(query.aggregations)
    nsel = query.num_select_aggs if query.num_select_aggs >= 0 else len(fns)
    if not query.group_by:
        return [[final_value(f, v) for f, v in zip(fns, res.row)][:nsel]]
    rows = [(k, [final_value(f, v) for f, v in zip(fns, vals)]) for k, vals in res.groups.items()]
    if query.order_by:
        rows.sort(key=_order_key_fn(query))
    else:
        rows.sort(key=lambda r: r[0])
    rows = rows[: query.limit]
    sel = query.select_columns
    out = []
    for k, vals in rows:
        out.append([k[query.group_by.index(c)] for c in sel] + vals[:nsel])
    return out


def merge_distinct(results, query: Q.Query):
    """Broker reduce of a distinct query (DistinctDataTableReducer.java:56,122 over DistinctTable.mergeTable): `results`
    are the servers' DistinctResults (engine.DistinctExecutor). The value records of all servers, each once, under the
    completed order (distinct.completed_order), cut at the limit alone (the offset is not applied, as in the reference).
    Returns (column names, rows)."""
    from . import distinct as D
    results = list(results)
    if not results:
        return list(query.select_columns), []
    cols, types = list(results[0].columns), list(results[0].column_types)
    for r in results[1:]:
        if list(r.columns) != cols:
            raise ValueError("servers disagree on the distinct columns")
    seen, records = set(), []
    for r in results:
        for row in r.rows:
            k = tuple(S_key(v, dt) for v, dt in zip(row, types))
            if k not in seen:
                seen.add(k)
                records.append(list(row))
    rows = D.sort_records(records, types, D.completed_order(query))
    return cols, rows[:int(query.limit)]


def S_key(value, data_type):
    """A record component as a hashable key that is equal exactly when the reference's values are (Double.compare
    equality for floating values)."""
    from . import selection as S
    return S.row_sort_key(value, data_type)


def merge_selection(results, query: Q.Query):
    """Broker reduce of a selection: `results` are the servers' SelectionResults (engine.SelectionExecutor) in server
    order, each sorted by the ORDER BY comparator. Merges them under that comparator (ties: server order, then the
    server's own row order — the sort is stable), drops `offset` rows, keeps `limit`, and projects the rows to the select
    list's order (`*`: the result's columns by name). Returns (column names, rows). Without ORDER BY the rows of the
    servers are concatenated in server order (SelectionOperatorService.reduceWithoutOrdering)."""
    from . import selection as S
    results = list(results)
    if not results:
        return [], []
    cols, types = results[0].columns, results[0].column_types
    for r in results[1:]:
        if list(r.columns) != list(cols):
            raise ValueError("servers disagree on the selection's columns")
    rows = [row for r in results for row in r.rows]
    # stable sorts from the least significant ORDER BY column up
    for ob in reversed(query.order_by):
        i = cols.index(ob.expr)
        rows.sort(key=lambda row, i=i, dt=types[i]: S.row_sort_key(row[i], dt), reverse=not ob.asc)
    rows = rows[query.offset: query.offset + query.limit]
    names = S.select_list(query, cols)
    idx = [cols.index(c) for c in names]
    return names, [[row[i] for i in idx] for row in rows]
