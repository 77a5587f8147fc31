"""GPU segment residency + query execution through the C-ABI.

Host-side mirror of the Java operator layer that stays in the JVM in a real integration:
  GpuSegment            ~ ImmutableSegmentLoader handing forward-index PinotDataBuffers to the GPU
  GpuQueryExecutor      ~ AggregationPlanNode/GroupByPlanNode -> AggregationOperator / GroupByOperator on every
                          segment + AggregationCombineOperator / GroupByCombineOperator
                          (pinot-core/.../operator/query/GroupByOperator.java:84,
                           operator/combine/GroupByCombineOperator.java:110)
It resolves predicates per segment (predicate.py), builds the table-wide group-key dictionaries (the value-keyed
merge GroupByCombineOperator performs with IndexedTable.upsert), and decodes the GPU's accumulators into the
reference's intermediate results: COUNT -> long, SUM/MIN/MAX -> double, AVG -> (sum, count),
DISTINCTCOUNTHLL -> HyperLogLog, PERCENTILE -> ValueHistogram (the DoubleArrayList as a multiset).
"""
import ctypes
import dataclasses
import threading
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np

from . import _lib as L
from . import predicate as P
from . import query as Q
from . import transform as T
from .hll import HyperLogLog, hash_value
from .java_hash import java_hash_code
from .optimizer import optimize_filter
from .segment import Segment

_VTYPE = {"INT": L.PA_INT, "LONG": L.PA_LONG, "FLOAT": L.PA_FLOAT, "DOUBLE": L.PA_DOUBLE, "STRING": L.PA_STRING}


class UnsupportedQuery(L.PinotAmdError):
    pass


def column_ids_for(segment: Segment) -> Dict[str, int]:
    """Table-level column id assignment (stable across the segments of one table)."""
    return {name: i for i, name in enumerate(sorted(segment.columns))}


class GpuSegment:
    """HBM-resident forward indexes + dictionaries of one immutable segment (a pa_segment)."""

    def __init__(self, segment: Segment, columns=None, column_ids=None, device=None):
        lib = L.lib()
        if device is not None:
            L.check(lib.pa_set_device(int(device)), "pa_set_device")
        self.device = None if device is None else int(device)  # (None: the caller's current device)
        self.segment = segment
        self.column_ids = dict(column_ids or column_ids_for(segment))
        self.handle = L.check_ptr(lib.pa_segment_create(segment.num_docs), "pa_segment_create")
        self._keep = []
        if segment.num_docs == 0:
            return  # an empty segment has no column indexes (SegmentColumnarIndexCreator.java:124 writes none)
        for name in (columns if columns is not None else segment.columns):
            self._add(name)

    def _add(self, name):
        lib = L.lib()
        col = self.segment.column(name)
        cid = self.column_ids[name]
        vt = _VTYPE[col.data_type]
        if col.has_dictionary:
            hashes = None
            if col.data_type in ("INT", "LONG"):
                dv = np.ascontiguousarray(col.dictionary, dtype=np.int64)
            elif col.data_type in ("FLOAT", "DOUBLE"):
                dv = np.ascontiguousarray(col.dictionary, dtype=np.float64)
            else:
                dv = None
                hashes = np.array([hash_value(v, "STRING") for v in col.dictionary.tolist()], dtype=np.int32)
            fwd = np.ascontiguousarray(col.fwd_bytes, dtype=np.uint8)
            if col.single_value:
                L.check(lib.pa_segment_add_sv_dict_column(
                    self.handle, cid, fwd.ctypes.data, fwd.nbytes, col.num_bits, col.cardinality, vt,
                    None if dv is None else dv.ctypes.data, None if hashes is None else hashes.ctypes.data),
                    "pa_segment_add_sv_dict_column(%s)" % name)
            else:
                L.check(lib.pa_segment_add_mv_dict_column(
                    self.handle, cid, fwd.ctypes.data, fwd.nbytes, col.num_bits, col.cardinality,
                    col.total_num_values, vt, None if dv is None else dv.ctypes.data,
                    None if hashes is None else hashes.ctypes.data),
                    "pa_segment_add_mv_dict_column(%s)" % name)
        else:
            raw = np.ascontiguousarray(col.raw_values)
            L.check(lib.pa_segment_add_raw_column(self.handle, cid, vt, raw.ctypes.data),
                    "pa_segment_add_raw_column(%s)" % name)

    @property
    def device_bytes(self):
        return int(L.lib().pa_segment_device_bytes(self.handle))

    def close(self):
        if self.handle:
            L.lib().pa_segment_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class AvgPair:
    """AvgAggregationFunction intermediate result (sum, count)."""
    sum: float
    count: int


@dataclass
class MinMaxRangePair:
    """MinMaxRangeAggregationFunction intermediate result (MinMaxRangePair: min, max; empty = (+inf, -inf))."""
    min: float
    max: float


@dataclass
class ValueTimePair:
    """FirstWithTime / LastWithTimeAggregationFunction intermediate result (ValueLongPair: the winning doc's value in
    the declared type — an int for 'BOOLEAN', as IntLongPair — and its time). The empty pair is the reference's
    DEFAULT_VALUE_TIME_PAIR (with_time_default)."""
    value: object
    time: int

    def __eq__(self, other):  # (NaN values of two default pairs compare equal)
        if not isinstance(other, ValueTimePair) or self.time != other.time:
            return False
        a, b = self.value, other.value
        return a == b or (isinstance(a, float) and isinstance(b, float) and a != a and b != b)


@dataclass
class VarianceTuple:
    """VarianceAggregationFunction intermediate result (VarianceTuple.java: count, sum, m2 = the sum of squared
    deviations from the mean). The empty tuple is (0, 0.0, 0.0)."""
    count: int
    sum: float
    m2: float


@dataclass
class CovarianceTuple:
    """CovarianceAggregationFunction intermediate result (CovarianceTuple.java: the raw sums of x, y and x * y, and the
    count, in the constructor's order). The empty tuple is (0.0, 0.0, 0.0, 0)."""
    sum_x: float
    sum_y: float
    sum_xy: float
    count: int


LONG_MIN, LONG_MAX = -(1 << 63), (1 << 63) - 1
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


def with_time_default(function, data_type):
    """DEFAULT_VALUE_TIME_PAIR of {First,Last}{Int,Long,Float,Double,String}ValueWithTimeAggregationFunction: the value
    Integer.MIN_VALUE / Long.MIN_VALUE / NaN / "", the time Long.MIN_VALUE for LAST and Long.MAX_VALUE for FIRST."""
    value = {"BOOLEAN": INT_MIN, "INT": INT_MIN, "LONG": LONG_MIN, "FLOAT": float("nan"), "DOUBLE": float("nan"),
             "STRING": ""}[data_type]
    return ValueTimePair(value, LONG_MIN if function == "LASTWITHTIME" else LONG_MAX)


def java_cast(value, stored_type, declared_type):
    """A stored value read through the BlockValSet getter of the declared type (getIntValuesSV / getLongValuesSV /
    getFloatValuesSV / getDoubleValuesSV over an INT / LONG / FLOAT / DOUBLE column): Java's primitive casts. long -> int
    keeps the low 32 bits; float / double -> int / long saturates, NaN -> 0; 'BOOLEAN' reads the int."""
    if declared_type == "STRING":
        if stored_type != "STRING":
            raise UnsupportedQuery("'STRING' over the %s column" % stored_type)
        return str(value)
    if stored_type not in ("INT", "LONG", "FLOAT", "DOUBLE"):
        raise UnsupportedQuery("'%s' over the %s column" % (declared_type, stored_type))
    floating = stored_type in ("FLOAT", "DOUBLE")
    if declared_type in ("INT", "BOOLEAN", "LONG"):
        lo, hi = (INT_MIN, INT_MAX) if declared_type != "LONG" else (LONG_MIN, LONG_MAX)
        if floating:
            x = float(value)
            if x != x:
                return 0
            return hi if x >= hi else (lo if x <= lo else int(x))
        v = int(value)
        if declared_type != "LONG":
            v = ((v + (1 << 31)) & 0xffffffff) - (1 << 31)
        return v
    if declared_type == "FLOAT":
        with np.errstate(over="ignore"):  # (a double past Float.MAX_VALUE casts to infinity)
            return float(np.float32(value))
    return float(value)


class ValueHistogram:
    """PercentileAggregationFunction / PercentileMVAggregationFunction intermediate result: the reference's
    DoubleArrayList of every aggregated value, held as a multiset: `values` float64 strictly ascending, `counts` int64
    (> 0) how often each was aggregated. merge = DoubleArrayList.addAll = counts added per value; the final result is
    the value at the percentile's rank of the sorted list."""
    __slots__ = ("values", "counts")

    def __init__(self, values=(), counts=()):
        self.values = np.asarray(values, dtype=np.float64)
        self.counts = np.asarray(counts, dtype=np.int64)
        assert self.values.shape == self.counts.shape and self.values.ndim == 1

    @classmethod
    def from_values(cls, values):
        """The multiset of a sequence of values."""
        v, c = np.unique(np.asarray(values, dtype=np.float64), return_counts=True)
        return cls(v, c)

    @property
    def total(self):
        return int(self.counts.sum())

    def merge(self, other):
        if not len(other.values):
            return ValueHistogram(self.values, self.counts)
        v, inv = np.unique(np.concatenate([self.values, other.values]), return_inverse=True)
        c = np.zeros(len(v), dtype=np.int64)
        np.add.at(c, inv, np.concatenate([self.counts, other.counts]))
        return ValueHistogram(v, c)

    def value_at(self, percentile):
        """PercentileAggregationFunction.extractFinalResult: -inf (DEFAULT_FINAL_RESULT) for no values, else the sorted
        values' element size - 1 at 100, (int) ((long) size * percentile / 100) otherwise."""
        size = self.total
        if size == 0:
            return float("-inf")
        rank = size - 1 if percentile == 100 else int(float(size) * float(percentile) / 100)
        rank = min(rank, size - 1)
        return float(self.values[int(np.searchsorted(np.cumsum(self.counts), rank, side="right"))])

    def __eq__(self, other):
        return (isinstance(other, ValueHistogram) and np.array_equal(self.values, other.values) and
                np.array_equal(self.counts, other.counts))

    def __repr__(self):
        return "ValueHistogram(%d values, %d distinct)" % (self.total, len(self.values))


@dataclass
class IntermediateResult:
    """What the server returns for the segment set (AggregationResultsBlock / GroupByResultsBlock contents)."""
    aggregations: List[Q.Aggregation]
    group_by: List[str]
    groups: Dict[tuple, list] = field(default_factory=dict)   # group-by: key values -> intermediate values
    row: Optional[list] = None                                # aggregation-only
    num_docs_scanned: int = 0
    num_total_docs: int = 0
    num_groups_limit_reached: bool = False
    # DataTable execution statistics (fetch(execution_stats=True); filter_stats.py)
    num_entries_scanned_in_filter: int = 0
    num_entries_scanned_post_filter: int = 0


class PinnedPool:
    """Page-locked host buffers (pa_host_alloc) reused across fetches: pa_query_fetch DMAs every result column straight
    into them. Arrays handed out are views, valid until the pool's next fetch from the same thread. One pool per thread
    (OUTPUT_POOL is thread-local), so concurrent fetches from different threads never share a buffer; a slot that grows
    retires its old buffer instead of freeing it (views an earlier fetch returned stay readable until close())."""

    def __init__(self):
        self.bufs = {}  # slot -> (address, bytes)
        self.retired = []

    def array(self, slot, count, dtype):
        dt = np.dtype(dtype)
        need = max(16, int(count) * dt.itemsize)
        addr, size = self.bufs.get(slot, (None, 0))
        if size < need:
            if addr:
                self.retired.append(addr)
            size = max(need, size * 2)
            addr = L.check_ptr(L.lib().pa_host_alloc(size), "pa_host_alloc")
            self.bufs[slot] = (addr, size)
        raw = np.ctypeslib.as_array((ctypes.c_uint8 * size).from_address(addr))
        return raw[:int(count) * dt.itemsize].view(dt)

    def close(self):
        for addr, _ in self.bufs.values():
            L.lib().pa_host_free(addr)
        for addr in self.retired:
            L.lib().pa_host_free(addr)
        self.bufs = {}
        self.retired = []


class _ThreadPools(threading.local):
    """OUTPUT_POOL: one PinnedPool per thread (attribute access forwards to this thread's pool)."""

    def __init__(self):
        self.pool = PinnedPool()

    def array(self, slot, count, dtype):
        return self.pool.array(slot, count, dtype)

    def close(self):
        self.pool.close()


OUTPUT_POOL = _ThreadPools()


def _flatten_filter(f, leaves, ops):
    """Filter tree -> leaves + postfix program (PA_OP_*)."""
    if isinstance(f, (Q.And, Q.Or)):
        for i, c in enumerate(f.children):
            _flatten_filter(c, leaves, ops)
            if i:
                ops.append(L.PA_OP_AND if isinstance(f, Q.And) else L.PA_OP_OR)
    elif isinstance(f, Q.Not):
        _flatten_filter(f.child, leaves, ops)
        ops.append(L.PA_OP_NOT)
    else:
        ops.append(L.PA_OP_LEAF | (len(leaves) << 8))
        leaves.append(f)


class GpuQueryExecutor:
    def __init__(self, query: Q.Query, gpu_segments: List[GpuSegment], flags=0, enforce_num_groups_limit=True,
                 table_dicts=None, wide_sum_columns=(), value_dicts=None, hash_keys_bound=0, schema=None,
                 tuning=None, moments=None):
        """table_dicts: optional {group-by column: sorted unique values} — the table-wide dictionary every rank of a
        multi-GPU query must share so that key ids address the same accumulator rows everywhere
        (parallel.table_layout builds it); by default it is the union of these segments' dictionaries.
        wide_sum_columns: columns whose SUM keeps the 64-bit (PA_AGGF_WIDE_SUM) accumulator layout even if these
        segments' values all fit int32 — agreed across ranks by parallel.table_layout.
        value_dicts: optional {DISTINCTCOUNT column: sorted unique values} — the table-wide value dictionary whose ids
        the presence bytes index (every rank of a multi-GPU query must share it); by default the union of these
        segments' dictionaries.
        hash_keys_bound: hashed key spaces: size the slot table for at least this many keys (parallel.table_layout
        agrees on the largest rank's bound so every rank's table can take its share of the cross-GPU merge).
        schema: {column: (data type, has dictionary, single value)} agreed across ranks (parallel.table_layout): when
        every segment given here is empty, the executor plans over a one-doc placeholder segment of that schema and never
        scans it, so the rank still holds a (zero) accumulator block of the agreed layout and joins the cross-GPU merge.
        tuning: optional {name: int} planner overrides of this query (pa_query_set_tuning; csrc/pa_tuning.h lists them):
        tests and measurement only.
        moments: optional {(column, second column or None): (form, pivot or None)} — the form (_lib.PA_MOMENTS_FORM_*) and
        the double form's pivot of a VAR / STDDEV / COVAR accumulator, agreed across ranks by parallel.table_layout
        (pa_query_set_moments); by default the library chooses both from these segments."""
        if not gpu_segments:
            raise ValueError("no segments")
        self.table_dicts = table_dicts or {}
        self.table_value_dicts = value_dicts or {}
        self.wide_sum_columns = set(wide_sum_columns or ())
        self.hash_keys_bound = int(hash_keys_bound or 0)
        self.moments = dict(moments or {})
        self.query = query
        # empty segments hold no indexes and contribute nothing but their (zero) doc count: only the others are bound
        self.all_segs = [g.segment for g in gpu_segments]
        self.gsegs = [g for g in gpu_segments if g.segment.num_docs > 0]
        self.segs = [g.segment for g in self.gsegs]
        self.device = next((g.device for g in gpu_segments if g.device is not None), None)
        self.flags = flags
        self.tuning = dict(tuning or {})
        self.enforce_num_groups_limit = enforce_num_groups_limit
        self.handle = None
        self.placeholder = None
        self.match_none = False  # the rewritten filter is FALSE: the block stays reset, nothing is scanned
        if not self.segs and schema:
            self.placeholder = GpuSegment(self._placeholder_segment(schema), column_ids=gpu_segments[0].column_ids,
                                          device=self.device)
            self.gsegs = [self.placeholder]
            self.segs = [self.placeholder.segment]
        if self.segs:
            self._plan()
        if self.placeholder is not None:
            self.segs = []  # (nothing to scan; the plan only fixes the accumulator layout)

    def _placeholder_segment(self, schema):
        """One doc per column of the agreed schema: dictionary columns hold one value of the agreed table-wide dictionary
        (group-by and DISTINCTCOUNT columns) or a zero, raw columns a zero, multi-value columns one value."""
        from .segment import create_segment
        data, types, raw, mv = {}, {}, [], []
        for name in Q.query_columns(self.query):
            dt, has_dict, sv = schema[name]
            d = self.table_dicts.get(name)
            if d is None:
                d = self.table_value_dicts.get(name)
            v = np.asarray(d)[:1] if d is not None and len(d) else np.array(["" if dt == "STRING" else 0])
            v = v.astype({"INT": np.int32, "LONG": np.int64, "FLOAT": np.float32, "DOUBLE": np.float64}.get(dt, object))
            data[name] = v if sv else [v]
            types[name] = dt
            if not has_dict:
                raw.append(name)
            if not sv:
                mv.append(name)
        return create_segment("placeholder", data, types, no_dictionary_columns=raw, multi_value_columns=mv)

    # ------------------------------------------------------------------ planning
    def _plan(self):
        lib = L.lib()
        ids = self.gsegs[0].column_ids
        seg0 = self.segs[0]
        # the reference's compile-time filter rewrites (QueryOptimizer: merged ranges / IN lists, constant predicates),
        # so the leaves below and the execution statistics follow the operator tree the reference builds
        schema = {n: (c.data_type, bool(c.single_value)) for n, c in seg0.columns.items()}
        filt = optimize_filter(self.query.filter, schema)
        if isinstance(filt, Q.BoolFilter):
            self.match_none = not filt.value  # FALSE: EmptyFilterOperator, TRUE: MatchAllFilterOperator
            filt = None
        if _has_comparison(filt):
            raise UnsupportedQuery("comparison between two different columns")
        self.query = dataclasses.replace(self.query, filter=filt)
        q = self.query
        spec = L.QuerySpec()

        # aggregations -> GPU accumulators (AVG = SUM + group count, AVGMV = SUM + COUNT_MV over the MV column; the
        # *MV forms aggregate every value of a multi-value column)
        self.pa_aggs = []
        self.agg_map = []
        # aggregation filters (AGG(x) FILTER (WHERE f)): one lane per distinct filter as written — the reference keys
        # its swim lanes by FilterContext (AggregationFunctionUtils.java:340-373), and QueryOptimizer.optimize
        # (QueryOptimizer.java:59-75) rewrites only the WHERE expression, never a FILTER clause, so no merge of ranges
        # or IN lists happens here either; only constants are folded. lane_dev[k]: the library's filter index of lane k,
        # or "all" (the filter folds to TRUE: its aggregations run in the main lane) / "none" (FALSE: a lane without docs,
        # its aggregations keep their empty values and never reach the GPU).
        self.lane_filters, self.lane_dev, self.dev_filters = [], [], []
        self.pa_agg_filter = []   # per GPU accumulator: the library's filter index, -1 = the main lane
        self.agg_lane = []        # per query aggregation: its lane (index into lane_filters), -1 = no filter
        acc_keys = []

        def lane_of(a):
            if a.filter is None:
                return -1
            if a.filter not in self.lane_filters:
                f = _fold_constants(a.filter)
                if _has_comparison(f):
                    raise UnsupportedQuery("comparison between two different columns in an aggregation filter")
                if isinstance(f, Q.BoolFilter):
                    dev = "all" if f.value else "none"
                else:
                    if len(self.dev_filters) == L.PA_MAX_AGG_FILTERS:
                        raise UnsupportedQuery("more than %d aggregation filters in one query" % L.PA_MAX_AGG_FILTERS)
                    self.dev_filters.append(f)
                    dev = len(self.dev_filters) - 1
                self.lane_filters.append(a.filter)
                self.lane_dev.append(dev)
            return self.lane_filters.index(a.filter)

        cur = [-1]  # the library's filter index of the aggregation being mapped

        def acc_index(key):
            ident = key + (cur[0],)
            if ident not in acc_keys:
                acc_keys.append(ident)
                self.pa_aggs.append(key)
                self.pa_agg_filter.append(cur[0])
            return acc_keys.index(ident)

        # transform expressions (SUM(ADD(a, b)), GROUP BY timeConvert(...); transform.py): every distinct expression of
        # the aggregation arguments and group-by items becomes one device program over a shared operand-column table
        # (pa_query_set_expressions). An expression aggregation's GPU accumulator is keyed by column id -2 - its index.
        for a in q.aggregations:
            if a.function in Q.MOMENT_FUNCTIONS:
                self._check_moments(a)
        self.exprs, self.programs, self.expr_columns = T.check_query(
            q, {n: (c.data_type, bool(c.single_value)) for n, c in seg0.columns.items()})
        expr_index = self.exprs.index

        for a in q.aggregations:
            fn = a.function
            if fn in Q.MOMENT_FUNCTIONS:
                self.agg_lane.append(-1)
                cur[0] = -1
                # keyed by the argument column(s): the spellings of one family over the same argument(s) share the
                # accumulator (third field: the covariance's second column id, -1 = variance)
                self.agg_map.append(acc_index((L.PA_AGG_MOMENTS, ids[a.column],
                                               ids[a.column2] if a.column2 is not None else -1)))
                continue
            if isinstance(a.column, Q.Expr):
                cid = -2 - expr_index(a.column)
                self.agg_lane.append(-1)
                cur[0] = -1
                if fn in ("SUM", "AVG"):
                    self.agg_map.append(acc_index((L.PA_AGG_SUM, cid, 0)))
                elif fn == "MIN":
                    self.agg_map.append(acc_index((L.PA_AGG_MIN, cid, 0)))
                elif fn == "MAX":
                    self.agg_map.append(acc_index((L.PA_AGG_MAX, cid, 0)))
                else:
                    self.agg_map.append((acc_index((L.PA_AGG_MIN, cid, 0)), acc_index((L.PA_AGG_MAX, cid, 0))))
                continue
            if fn in Q.WITH_TIME_FUNCTIONS:
                self._check_with_time(a)
                self.agg_lane.append(-1)
                cur[0] = -1
                # keyed by (type, time column): the accumulator knows nothing of the value column, so aggregations
                # over one time column share it
                t = L.PA_AGG_LAST_ROW_BY_TIME if fn == "LASTWITHTIME" else L.PA_AGG_FIRST_ROW_BY_TIME
                self.agg_map.append(acc_index((t, ids[a.time_column], 0)))
                continue
            if fn.endswith("MV") and seg0.column(a.column).single_value:
                raise UnsupportedQuery("%s on single-value column %s" % (fn, a.column))
            lane = lane_of(a)
            self.agg_lane.append(lane)
            dev = self.lane_dev[lane] if lane >= 0 else "all"
            if dev == "none":
                self.agg_map.append(None)  # (fetch fills in the function's empty value)
                continue
            cur[0] = -1 if dev == "all" else dev
            if fn == "COUNT":
                self.agg_map.append(acc_index((L.PA_AGG_COUNT, -1, 0)))
            elif fn == "AVGMV":
                self.agg_map.append((acc_index((L.PA_AGG_SUM, ids[a.column], 0)),
                                     acc_index((L.PA_AGG_COUNT_MV, ids[a.column], 0))))
            elif fn == "COUNTMV":
                self.agg_map.append(acc_index((L.PA_AGG_COUNT_MV, ids[a.column], 0)))
            elif fn in ("SUM", "AVG", "SUMMV"):
                self.agg_map.append(acc_index((L.PA_AGG_SUM, ids[a.column], 0)))
            elif fn in ("MIN", "MINMV"):
                self.agg_map.append(acc_index((L.PA_AGG_MIN, ids[a.column], 0)))
            elif fn in ("MAX", "MAXMV"):
                self.agg_map.append(acc_index((L.PA_AGG_MAX, ids[a.column], 0)))
            elif fn in Q.HLL_FUNCTIONS:
                self.agg_map.append(acc_index((L.PA_AGG_DISTINCTCOUNTHLL, ids[a.column], a.log2m)))
            elif fn in ("MINMAXRANGE", "MINMAXRANGEMV"):
                # MinMaxRangePair(min, max): the MIN and MAX accumulators of the column
                self.agg_map.append((acc_index((L.PA_AGG_MIN, ids[a.column], 0)),
                                     acc_index((L.PA_AGG_MAX, ids[a.column], 0))))
            elif fn in Q.DISTINCT_SET_FUNCTIONS:
                if not all(sg.column(a.column).has_dictionary for sg in self.segs):
                    raise UnsupportedQuery("%s on a raw (no-dictionary) column %s" % (fn, a.column))
                self.agg_map.append(acc_index((L.PA_AGG_DISTINCTCOUNT, ids[a.column], 0)))
            elif fn in Q.PERCENTILE_FUNCTIONS:
                # one value histogram per column, whatever percentiles of it the query asks for
                if not all(sg.column(a.column).has_dictionary for sg in self.segs):
                    raise UnsupportedQuery("%s on a raw (no-dictionary) column %s" % (fn, a.column))
                if seg0.column(a.column).data_type not in ("INT", "LONG", "FLOAT", "DOUBLE"):
                    raise UnsupportedQuery("%s on the %s column %s" % (fn, seg0.column(a.column).data_type, a.column))
                self.agg_map.append(acc_index((L.PA_AGG_VALUE_HISTOGRAM, ids[a.column], 0)))
            else:
                raise UnsupportedQuery("aggregation %s" % fn)
        if q.aggregations and all(m is None for m in self.agg_map):
            self.match_none = True  # every aggregation's filter is FALSE: no lane sees a doc, so no group exists
            self.pa_aggs.append((L.PA_AGG_COUNT, -1, 0))  # (the block's layout only: nothing is scanned)
            self.pa_agg_filter.append(-1)
        if len(self.pa_aggs) > L.PA_MAX_AGGS:
            raise UnsupportedQuery("too many aggregations")
        spec.num_aggs = len(self.pa_aggs)
        names = {cid: name for name, cid in ids.items()}
        # DISTINCTCOUNT: the table-wide value dictionary of the column (presence byte j <=> value value_dicts[j]);
        # PERCENTILE's value histogram: the same dictionary (bin j <=> value value_dicts[j])
        self.value_dicts = {}
        for i, (t, cid, log2m) in enumerate(self.pa_aggs):
            spec.aggs[i].type = t
            spec.aggs[i].column_id = max(cid, 0)
            spec.aggs[i].log2m = log2m if t != L.PA_AGG_MOMENTS else 0
            if t == L.PA_AGG_SUM and names.get(cid) in self.wide_sum_columns:
                spec.aggs[i].flags = L.PA_AGGF_WIDE_SUM
            time_dict = t in TIME_ROW_AGGS and self.segs[0].column(names[cid]).has_dictionary
            if t in (L.PA_AGG_DISTINCTCOUNT, L.PA_AGG_VALUE_HISTOGRAM) or time_dict:
                # (a dictionary time column of FIRSTWITHTIME / LASTWITHTIME: its table-wide dictionary, ids in value order)
                name = names[cid]
                if name in self.table_value_dicts:
                    vd = np.asarray(self.table_value_dicts[name])
                else:
                    ds = [sg.column(name).dictionary for sg in self.segs]
                    same = all(d is ds[0] or (len(d) == len(ds[0]) and np.array_equal(d, ds[0])) for d in ds)
                    vd = ds[0] if same else np.unique(np.concatenate(ds))
                self.value_dicts[i] = vd
                spec.aggs[i].num_values = len(vd)

        # filter
        filt = q.filter
        leaves, ops = [], []
        if filt is not None:
            _flatten_filter(filt, leaves, ops)
        # the aggregation filters' leaves follow the main filter's (pa_query_set_agg_filters): bound per segment below
        # like any other leaf; each filter has its own postfix program
        self.dev_filter_ops = []
        for f in self.dev_filters:
            fops = []
            _flatten_filter(f, leaves, fops)
            self.dev_filter_ops.append(fops)
        if len(leaves) > L.PA_MAX_LEAVES or len(ops) > L.PA_MAX_OPS or any(len(o) > L.PA_MAX_OPS for o in self.dev_filter_ops):
            raise UnsupportedQuery("filter too large" if not self.dev_filters else
                                   "filters too large: the WHERE and the aggregation filters hold more than %d leaves "
                                   "together, or one of them more than %d operations" % (L.PA_MAX_LEAVES, L.PA_MAX_OPS))
        per_seg = []
        for seg in self.segs:
            params = []
            for pred in leaves:
                col = seg.column(pred.column)
                params.append(P.dictionary_leaf(pred, col) if col.has_dictionary else P.raw_leaf(pred, col))
            per_seg.append(params)
        self.leaf_params = per_seg  # (also the execution statistics' leaf evaluators: filter_stats)
        spec.num_leaves = len(leaves)
        for li, pred in enumerate(leaves):
            kinds = {ps[li].kind for ps in per_seg}
            kind = L.PA_LEAF_DICT_SET if L.PA_LEAF_DICT_SET in kinds else kinds.pop()
            if not seg0.column(pred.column).single_value:  # MVScanDocIdIterator: ANY value (ALL for NOT IN / !=)
                kind = {L.PA_LEAF_DICT_RANGE: L.PA_LEAF_MV_DICT_RANGE, L.PA_LEAF_DICT_SET: L.PA_LEAF_MV_DICT_SET}[kind]
            spec.leaves[li].column_id = ids[pred.column]
            spec.leaves[li].kind = kind
        spec.num_ops = len(ops)
        for i, op in enumerate(ops):
            spec.ops[i] = op

        # group-by: table-wide dictionaries (value-keyed combine)
        self.global_dicts = []
        self.remaps = []  # [seg][gb] -> np.int32 or None
        spec.num_group_by = len(q.group_by)
        if spec.num_group_by > L.PA_MAX_GROUP_BY:
            raise UnsupportedQuery("too many group-by columns")
        self.raw_group_by = []
        self.group_by_expr = []  # per group-by position: its expression's index, or -1
        for j, name in enumerate(q.group_by):
            if isinstance(name, Q.Expr):
                # grouped by the value's 64 bits, as a raw LONG / DOUBLE column is (NoDictionary*GroupKeyGenerator)
                e = expr_index(name)
                self.group_by_expr.append(e)
                self.global_dicts.append(None)
                self.raw_group_by.append(self.programs[e].result_type)
                spec.group_by_columns[j] = 0
                spec.group_by_cardinality[j] = 0
                continue
            self.group_by_expr.append(-1)
            has_dict = [s.column(name).has_dictionary for s in self.segs]
            if not any(has_dict):
                # raw (no-dictionary) column: grouped by value through the hashed key space
                # (NoDictionarySingleColumnGroupKeyGenerator / NoDictionaryMultiColumnGroupKeyGenerator)
                self.global_dicts.append(None)
                self.raw_group_by.append(seg0.column(name).data_type)
                spec.group_by_columns[j] = ids[name]
                spec.group_by_cardinality[j] = 0
                continue
            if not all(has_dict):
                raise UnsupportedQuery("group-by column %s is dictionary-encoded in some segments only" % name)
            self.raw_group_by.append(None)
            dicts = [s.column(name).dictionary for s in self.segs]
            if name in self.table_dicts:
                gd = np.asarray(self.table_dicts[name])
                if not all(np.isin(d, gd).all() for d in dicts):
                    raise ValueError("table dictionary of %s misses values of a bound segment" % name)
            else:
                first = dicts[0]
                same = all(d is first or (len(d) == len(first) and np.array_equal(d, first)) for d in dicts)
                gd = first if same else np.unique(np.concatenate(dicts))
            self.global_dicts.append(gd)
            spec.group_by_columns[j] = ids[name]
            spec.group_by_cardinality[j] = len(gd)
        for seg in self.segs:
            rm = []
            for j, name in enumerate(q.group_by):
                gd = self.global_dicts[j]
                d = None if gd is None else seg.column(name).dictionary
                if gd is None or d is gd or (len(d) == len(gd) and np.array_equal(d, gd)):
                    rm.append(None)
                else:
                    rm.append(self._group_remap(name, gd, d))
            self.remaps.append(rm)
        spec.flags = ((self.flags & 0xffffffff) ^ 0x80000000) - 0x80000000  # (int32: PA_QF_NO_JIT is bit 31)
        spec.flags2 = (self.flags >> 32) & 0x7fffffff if self.flags >= 0 else 0
        spec.hash_keys_bound = self.hash_keys_bound

        # numGroupsLimit (DictionaryBasedGroupKeyGenerator._globalGroupIdUpperBound): the per-segment first-seen group
        # cap. The library decides whether it can bind and then runs the first-seen trimming passes on the GPU;
        # enforce_num_groups_limit=False drops the cap (measurement tools only: results then differ from the
        # reference whenever the cap binds).
        spec.num_groups_limit = int(min(q.num_groups_limit, 2**31 - 1)) if (q.group_by and self.enforce_num_groups_limit) else 0

        self.spec = spec
        self.handle = L.check_ptr(lib.pa_query_create(ctypes.byref(spec), len(self.segs)), "pa_query_create")
        for name, value in self.tuning.items():
            L.check(lib.pa_query_set_tuning(self.handle, name.encode(), int(value)), "pa_query_set_tuning")
        self._keep = []
        self._after_create()
        if self.exprs:
            if self.dev_filters:
                raise UnsupportedQuery("transform expressions next to aggregation filters")
            es = T.fill_spec(self.programs, [ids[c] for c in self.expr_columns],
                             [-2 - cid if cid <= -2 else -1 for _, cid, _ in self.pa_aggs], self.group_by_expr)
            L.check(lib.pa_query_set_expressions(self.handle, ctypes.byref(es)), "pa_query_set_expressions")
        if any(t == L.PA_AGG_MOMENTS for t, _, _ in self.pa_aggs):
            ms = L.MomentsSpec()
            for i in range(L.PA_MAX_AGGS):
                ms.second_column[i] = -1
            for i, (t, cid, cid2) in enumerate(self.pa_aggs):
                if t != L.PA_AGG_MOMENTS:
                    continue
                ms.second_column[i] = cid2
                form, pivot = self.moments.get((names[cid], names[cid2] if cid2 >= 0 else None), (L.PA_MOMENTS_FORM_AUTO, None))
                ms.form[i] = int(form)
                if pivot is not None and cid2 < 0:
                    ms.has_pivot[i] = 1
                    ms.pivot[i] = float(pivot)
            L.check(lib.pa_query_set_moments(self.handle, ctypes.byref(ms)), "pa_query_set_moments")
        if self.dev_filters:
            fs = L.AggFilterSpec()
            fs.num_filters = len(self.dev_filters)
            for j, fops in enumerate(self.dev_filter_ops):
                fs.num_ops[j] = len(fops)
                for i, op in enumerate(fops):
                    fs.ops[j][i] = op
            for i in range(L.PA_MAX_AGGS):
                fs.agg_filter[i] = self.pa_agg_filter[i] if i < len(self.pa_agg_filter) else -1
            L.check(lib.pa_query_set_agg_filters(self.handle, ctypes.byref(fs)), "pa_query_set_agg_filters")
        for si, (g, params) in enumerate(zip(self.gsegs, per_seg)):
            arr = (L.LeafParams * max(1, len(params)))()
            for li, p in enumerate(params):
                lp = arr[li]
                if isinstance(p, P.DictLeaf):
                    lp.negate = int(p.negate)
                    if spec.leaves[li].kind in (L.PA_LEAF_DICT_SET, L.PA_LEAF_MV_DICT_SET):
                        ids_ = p.ids if p.ids is not None else np.arange(p.lo, p.hi, dtype=np.int32)
                        lut = P.DictLeaf(L.PA_LEAF_DICT_SET, ids=ids_).lut_words(self.segs[si].column(leaves[li].column).cardinality)
                        self._keep.append(lut)
                        lp.lut = lut.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
                    else:
                        lp.lo, lp.hi = p.lo, p.hi
                else:
                    lp.negate = int(p.negate)
                    lp.ilo = max(min(int(p.ilo), P.LONG_MAX), P.LONG_MIN)
                    lp.ihi = max(min(int(p.ihi), P.LONG_MAX), P.LONG_MIN)
                    lp.dlo, lp.dhi = float(p.dlo), float(p.dhi)
                    if p.kind == L.PA_LEAF_RAW_SET:
                        vals = np.ascontiguousarray(p.values)
                        self._keep.append(vals)
                        lp.values = vals.ctypes.data if len(vals) else None
                        lp.num_values = len(vals)
            rms = (ctypes.c_void_p * max(1, len(q.group_by)))()
            for j, rm in enumerate(self.remaps[si]):
                if rm is not None:
                    self._keep.append(rm)
                    rms[j] = rm.ctypes.data
            L.check(lib.pa_query_bind_segment(self.handle, si, g.handle, arr, rms), "pa_query_bind_segment")
            for i, vd in self.value_dicts.items():
                d = self.segs[si].column(names[self.pa_aggs[i][1]]).dictionary
                if d is vd or (len(d) == len(vd) and np.array_equal(d, vd)):
                    continue
                if not np.isin(d, vd).all():
                    raise ValueError("table-wide value dictionary misses values of a bound segment")
                rm = np.searchsorted(vd, d).astype(np.int32)
                self._keep.append(rm)
                L.check(lib.pa_query_bind_value_remap(self.handle, si, i, rm.ctypes.data), "pa_query_bind_value_remap")
        self._before_prepare()
        try:
            L.check(lib.pa_query_prepare(self.handle), "pa_query_prepare")
        except L.PinotAmdError as e:
            with_time = any(a.function in Q.WITH_TIME_FUNCTIONS + Q.MOMENT_FUNCTIONS for a in q.aggregations)
            if (self.dev_filters or self.exprs or with_time) and getattr(e, "code", 0) == L.PA_EUNSUPPORTED:
                # (what the library refuses of a query with aggregation filters, transform expressions,
                # FIRSTWITHTIME / LASTWITHTIME or VAR / STDDEV / COVAR)
                raise UnsupportedQuery(str(e)) from None
            raise
        self.num_keys = int(lib.pa_query_num_keys(self.handle))
        hashed, shifts = ctypes.c_int32(), (ctypes.c_int32 * max(1, len(q.group_by)))()
        L.check(lib.pa_query_key_layout(self.handle, ctypes.byref(hashed), shifts), "pa_query_key_layout")
        self.hashed = bool(hashed.value)
        self.key_shifts = list(shifts)[:len(q.group_by)]
        self.key_words = int(lib.pa_query_key_words(self.handle))  # 2: two int64 per hashed key
        self.strides = []
        s = 1
        for gd in self.global_dicts:
            self.strides.append(s)
            s *= len(gd) if gd is not None else 1

    def _check_moments(self, a):
        """What VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP / COVAR_POP / COVAR_SAMP take here (DESIGN.md "Moments",
        limits); the key-space limits are the library's (pa_query_prepare: PA_EUNSUPPORTED)."""
        fn = a.function
        if a.filter is not None:
            raise UnsupportedQuery("%s with a FILTER (WHERE ...) clause" % fn)
        if any(b.filter is not None for b in self.query.aggregations):
            raise UnsupportedQuery("%s in a query with aggregation filters" % fn)
        if str(self.query.options.get("enableNullHandling", "false")).lower() == "true":
            raise UnsupportedQuery("%s with null handling" % fn)
        for c in (a.column,) + ((a.column2,) if fn in Q.COVARIANCE_FUNCTIONS else ()):
            if isinstance(c, Q.Expr):
                raise UnsupportedQuery("%s over a transform expression as its argument" % fn)
            for sg in self.segs:
                col = sg.column(c)
                if not col.single_value:
                    raise UnsupportedQuery("%s over the multi-value column %s" % (fn, c))
                if col.data_type not in ("INT", "LONG", "FLOAT", "DOUBLE"):
                    raise UnsupportedQuery("%s over the %s column %s" % (fn, col.data_type, c))

    def fetch_moments(self, pi, num_groups, stream=None):
        """The tuples of VAR / STDDEV / COVAR accumulator `pi` for the groups the last fetch_arrays returned, in its order
        (pa_query_fetch_moments): a list of VarianceTuple, or of CovarianceTuple for a covariance. Synchronises `stream`."""
        n = int(num_groups)
        count = np.zeros(max(n, 1), dtype=np.int64)
        vals = np.zeros((3, max(n, 1)), dtype=np.float64)
        if n:
            ptrs = (ctypes.c_void_p * 3)(*[vals[c].ctypes.data for c in range(3)])
            L.check(L.lib().pa_query_fetch_moments(self.handle, stream, pi, n, count.ctypes.data, ptrs),
                    "pa_query_fetch_moments")
        c_, v0, v1, v2 = count[:n].tolist(), vals[0, :n].tolist(), vals[1, :n].tolist(), vals[2, :n].tolist()
        if self.pa_aggs[pi][2] >= 0:
            return [CovarianceTuple(v0[r], v1[r], v2[r], c_[r]) for r in range(n)]
        return [VarianceTuple(c_[r], v0[r], v1[r]) for r in range(n)]

    def moments_form(self, pi):
        """(form, pivot) the library uses for VAR / STDDEV / COVAR accumulator `pi` (pa_query_moments_form)."""
        form, pivot = ctypes.c_int32(), ctypes.c_double()
        L.check(L.lib().pa_query_moments_form(self.handle, pi, ctypes.byref(form), ctypes.byref(pivot)),
                "pa_query_moments_form")
        return int(form.value), float(pivot.value)

    def _check_with_time(self, a):
        """What FIRSTWITHTIME / LASTWITHTIME takes here (DESIGN.md "First / last with time", limits); the key-space
        limits are the library's (pa_query_prepare: PA_EUNSUPPORTED)."""
        fn = a.function
        if a.filter is not None:
            raise UnsupportedQuery("%s with a FILTER (WHERE ...) clause" % fn)
        if str(self.query.options.get("enableNullHandling", "false")).lower() == "true":
            raise UnsupportedQuery("%s with null handling" % fn)
        for what, c in (("value", a.column), ("time", a.time_column)):
            if isinstance(c, Q.Expr):
                raise UnsupportedQuery("%s over a transform expression as its %s column" % (fn, what))
            for sg in self.segs:
                col = sg.column(c)
                if not col.single_value:
                    raise UnsupportedQuery("%s over the multi-value %s column %s" % (fn, what, c))
                if col.data_type == "BYTES":
                    raise UnsupportedQuery("%s over the BYTES %s column %s" % (fn, what, c))
        tcols = [sg.column(a.time_column) for sg in self.segs]
        if tcols[0].data_type not in ("INT", "LONG"):
            raise UnsupportedQuery("%s: the time column %s is %s, not INT or LONG" % (fn, a.time_column, tcols[0].data_type))
        if len({bool(c.has_dictionary) for c in tcols}) > 1:
            raise UnsupportedQuery("%s: the time column %s is dictionary-encoded in some segments only" % (fn, a.time_column))
        stored = self.segs[0].column(a.column).data_type
        if (a.data_type == "STRING") != (stored == "STRING"):
            raise UnsupportedQuery("%s: '%s' over the %s column %s" % (fn, a.data_type, stored, a.column))
        if not hasattr(self, "with_time_stored"):
            self.with_time_stored = {}  # value column -> stored type (fetch converts it to the declared type)
        self.with_time_stored[a.column] = stored

    def fetch_time_rows(self, pi, num_groups, columns, stream=None):
        """The winning rows of FIRSTWITHTIME / LASTWITHTIME accumulator `pi` for the groups the last fetch_arrays
        returned, in its order (pa_query_fetch_time_rows): (segments int32[n], docs int32[n], {column: values}) with every
        column's cell decoded through the winning segment's dictionary (a list of Python values; None for a group
        without a row, whose segment and doc are -1). Synchronises `stream`."""
        n = int(num_groups)
        ids = self.gsegs[0].column_ids
        segs = np.full(max(n, 1), -1, dtype=np.int32)
        docs = np.full(max(n, 1), -1, dtype=np.int32)
        cells = np.zeros((max(len(columns), 1), max(n, 1)), dtype=np.int64)
        if n:
            cids = (ctypes.c_int32 * max(1, len(columns)))(*[ids[c] for c in columns])
            ptrs = (ctypes.c_void_p * max(1, len(columns)))(*[cells[c].ctypes.data for c in range(len(columns))])
            L.check(L.lib().pa_query_fetch_time_rows(self.handle, stream, pi, n, len(columns), cids, segs.ctypes.data,
                                                     docs.ctypes.data, ptrs), "pa_query_fetch_time_rows")
        segs, docs = segs[:n], docs[:n]
        out = {}
        for c, name in enumerate(columns):
            vals = [None] * n
            for si, sg in enumerate(self.segs):
                rows = np.flatnonzero(segs == si)
                if not len(rows):
                    continue
                col = sg.column(name)
                cc = cells[c, rows]
                if col.has_dictionary:
                    got = np.asarray(col.dictionary)[cc].tolist()
                elif col.data_type in ("FLOAT", "DOUBLE"):  # (the bits of the value as a double)
                    got = cc.view(np.float64).tolist()
                else:
                    got = cc.tolist()
                for r, v in zip(rows.tolist(), got):
                    vals[r] = v
            out[name] = vals
        return segs, docs, out

    def _group_remap(self, name, table_dict, dictionary):
        """int32[len(dictionary)]: the table-wide key id of every value of a segment's dictionary of group-by column
        `name` (both ascending in numpy's order here; DistinctExecutor orders STRING columns as the reference does)."""
        return np.searchsorted(table_dict, dictionary).astype(np.int32)

    def _after_create(self):
        """Between pa_query_create and the first pa_query_bind_segment (SelectionExecutor sets the selection here)."""

    def _before_prepare(self):
        """After every segment is bound, before pa_query_prepare (SelectionExecutor binds its order remaps here)."""

    # ------------------------------------------------------------------ execution
    def execute(self, stream=None):
        if not self.segs or self.match_none:  # nothing to scan (a placeholder plan, a FALSE filter): block reset only
            if self.handle is not None:
                L.check(L.lib().pa_query_reset(self.handle, stream), "pa_query_reset")
            return
        L.check(L.lib().pa_query_execute(self.handle, stream), "pa_query_execute")
        self._scanned = True
        self.merged_stats = None

    def reset(self, stream=None):
        L.check(L.lib().pa_query_reset(self.handle, stream), "pa_query_reset")
        self._scanned = False
        self.merged_stats = None

    def scan(self, stream=None):
        if not self.segs or self.match_none:
            return
        L.check(L.lib().pa_query_scan(self.handle, stream), "pa_query_scan")
        self._scanned = True
        self.merged_stats = None

    def sections(self):
        """[(kind, device_ptr, num_elements)] accumulator sections (for the cross-GPU reduce)."""
        lib = L.lib()
        out = []
        for i in range(lib.pa_query_num_sections(self.handle)):
            kind, n = ctypes.c_int32(), ctypes.c_int64()
            p = L.check_ptr(lib.pa_query_section(self.handle, i, ctypes.byref(kind), ctypes.byref(n)), "section")
            out.append((kind.value, p, n.value))
        return out

    def stats(self):
        a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        L.check(L.lib().pa_query_stats(self.handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "stats")
        out = {"staged_bytes": a.value, "num_docs": b.value, "num_wave_tiles": c.value}
        vals = [ctypes.c_int32() for _ in range(7)]
        L.check(L.lib().pa_query_plan(self.handle, *[ctypes.byref(v) for v in vals]), "plan")
        names = ("strategy", "steps", "dma_slots", "ring", "wg_per_cu", "grid", "lds_bytes")
        out["plan"] = {n: v.value for n, v in zip(names, vals)}
        code = out["plan"]["strategy"]
        out["plan"]["strategy"] = {0: "lds", 1: "global", 2: "partitioned", 4: "lane", 5: "lane", 6: "lane", 7: "lane",
                                    8: "lds_dense", 9: "lds_dense", 10: "lds_dense", 11: "lds_dense", 12: "lds_dense",
                                    14: "lds_dense", 15: "lds_dense", 128: "select", 129: "distinct",
                                    130: "distinct", 131: "filtered", 132: "filtered", 133: "expr", 134: "expr",
                                    135: "time_rows", 136: "time_rows", 137: "moments", 138: "moments"}[code]
        out["plan"]["variant"] = STRATEGY_VARIANTS.get(code, str(code))
        out["plan"]["eager_literals"] = int(L.lib().pa_query_num_eager_literals(self.handle))
        out["plan"]["lane_major"] = int(L.lib().pa_query_lane_major(self.handle))
        out["plan"]["dense_packed"] = int(L.lib().pa_query_dense_packed(self.handle))
        out["plan"]["count_free_emit"] = int(L.lib().pa_query_count_free_emit(self.handle))
        out["plan"]["eq_prefilter"] = int(L.lib().pa_query_eq_prefilter(self.handle))
        out["plan"]["stream_nt"] = int(L.lib().pa_query_stream_nt(self.handle))
        out["plan"]["eq_jit"] = int(L.lib().pa_query_eq_jit(self.handle))
        out["plan"]["partition_keys"] = int(L.lib().pa_query_partition_keys(self.handle))
        out["plan"]["limit_trimming"] = int(L.lib().pa_query_limit_trimming(self.handle))
        out["plan"]["results_invalid"] = int(L.lib().pa_query_results_invalid(self.handle))
        # FIRSTWITHTIME / LASTWITHTIME accumulators: {accumulator index: 1 = packed, 2 = wide} (pa_query_time_row_form)
        out["plan"]["time_row_form"] = {i: int(L.lib().pa_query_time_row_form(self.handle, i))
                                        for i, (t, _, _) in enumerate(self.pa_aggs) if t in TIME_ROW_AGGS}
        # VAR / STDDEV / COVAR accumulators: {accumulator index: (form, pivot)} (pa_query_moments_form)
        out["plan"]["moments_form"] = {i: self.moments_form(i)
                                       for i, (t, _, _) in enumerate(self.pa_aggs) if t == L.PA_AGG_MOMENTS}
        return out

    def fetch_arrays(self, stream=None, pooled=False, trim_spec=None):
        """Non-empty groups in ascending table-wide key order as arrays: (keys int64[n], counts int64[n],
        [one array per GPU accumulator: float64[n], or uint8[n << log2m] HLL registers]). Synchronises `stream`.
        pooled=True: the arrays are views of the process's page-locked output pool (OUTPUT_POOL: each column arrives by
        one DMA; valid until the next pooled fetch of any executor) instead of fresh arrays.
        trim_spec (a _lib.TrimSpec, trim.build_spec): only the groups the server trim keeps, chosen on the GPU
        (pa_query_fetch_trimmed); self.trim_total_groups is then the number of non-empty groups."""
        lib = L.lib()
        alloc = (lambda slot, n, dt: OUTPUT_POOL.array(slot, n, dt)) if pooled else (lambda slot, n, dt: np.empty(n, dt))
        cap = 1 if not self.query.group_by else min(self.num_keys, 1 << 16)
        if trim_spec is not None:
            cap = max(1, min(self.num_keys, int(trim_spec.trim)))
            total = ctypes.c_int64(0)
        elif self.query.group_by and self.num_keys > 1 << 16:
            # large key space: a capacity-0 call runs only the GPU count pass and returns the number of non-empty
            # groups, so the gather + copy run once, at the exact size
            cap = max(1, L.check(lib.pa_query_fetch(self.handle, stream, 0, None, None, None), "pa_query_fetch"))
        kw = getattr(self, "key_words", 1)
        while True:
            keys = alloc("keys", cap * kw, np.int64)
            counts = alloc("counts", cap, np.int64)
            outs, ptrs = [], (ctypes.c_void_p * max(1, len(self.pa_aggs)))()
            for i, (t, _, log2m) in enumerate(self.pa_aggs):
                if t == L.PA_AGG_DISTINCTCOUNTHLL:
                    o = alloc(i, cap << log2m, np.uint8)
                elif t == L.PA_AGG_DISTINCTCOUNT:
                    o = alloc(i, cap * self._presence_stride(i), np.uint8)
                elif t == L.PA_AGG_VALUE_HISTOGRAM or t in TIME_ROW_AGGS or t == L.PA_AGG_MOMENTS:
                    # (pa_query_fetch writes nothing: fetch_histograms / percentiles read the bins, fetch_time_rows the rows,
                    # fetch_moments the tuples)
                    outs.append(None)
                    continue
                else:
                    o = alloc(i, cap, np.float64)
                outs.append(o)
                ptrs[i] = o.ctypes.data
            if trim_spec is not None:
                n = L.check(lib.pa_query_fetch_trimmed(self.handle, stream, ctypes.byref(trim_spec), cap,
                                                       keys.ctypes.data, counts.ctypes.data, ptrs, ctypes.byref(total)),
                            "pa_query_fetch_trimmed")
                self.trim_total_groups = int(total.value)
            else:
                n = L.check(lib.pa_query_fetch(self.handle, stream, cap, keys.ctypes.data, counts.ctypes.data, ptrs),
                            "pa_query_fetch")
            if n <= cap:
                break
            cap = n
        outs = [None if o is None else
                o[: n << self.pa_aggs[i][2]] if self.pa_aggs[i][0] == L.PA_AGG_DISTINCTCOUNTHLL else
                (o[: n * self._presence_stride(i)] if self.pa_aggs[i][0] == L.PA_AGG_DISTINCTCOUNT else o[:n])
                for i, o in enumerate(outs)]
        return (keys[:n] if kw == 1 else keys[:2 * n].reshape(n, 2)), counts[:n], outs

    def fetch_lane_counts(self, num_groups, stream=None):
        """int64[filters, num_groups]: the docs of every aggregation filter's lane (W AND F_j) in the groups the last
        fetch_arrays returned, in its order (pa_query_fetch_lane_counts). Synchronises `stream`."""
        nf = len(self.dev_filters)
        out = np.zeros((nf, max(int(num_groups), 1)), dtype=np.int64)[:, :int(num_groups)]
        out = np.ascontiguousarray(out)
        if nf and num_groups:
            L.check(L.lib().pa_query_fetch_lane_counts(self.handle, stream, int(num_groups), out.ctypes.data),
                    "pa_query_fetch_lane_counts")
        return out

    def lane_docs(self, stream=None):
        """int64[segments, 1 + filters]: per bound segment the docs matching the query's filter W, then W AND F_j for
        every aggregation filter (pa_query_lane_docs), of the last scan. After a fetch the library hands out the
        counters that fetch read (no further synchronisation). A query whose FILTER clauses all folded to constants
        has no lane on the device: its scan counted W's docs over all segments together (pa_query_matched_docs), so
        W's docs per segment are the segment's docs (no WHERE), that total (one segment), or the WHERE's mask over
        the GPU's leaf bitmaps (synchronises `stream`)."""
        out = np.zeros((len(self.segs), 1 + len(self.dev_filters)), dtype=np.int64)
        if not self.segs or self.match_none or self.handle is None or not getattr(self, "_scanned", False):
            return out
        if self.dev_filters:
            L.check(L.lib().pa_query_lane_docs(self.handle, out.ctypes.data), "pa_query_lane_docs")
        elif self.lane_filters:
            from . import filter_stats as FS
            if self.query.filter is None:
                out[:, 0] = [seg.num_docs for seg in self.segs]
            elif len(self.segs) == 1:
                out[0, 0] = int(L.lib().pa_query_matched_docs(self.handle))
            else:
                for si, seg in enumerate(self.segs):
                    out[si, 0] = int(FS.filter_mask(self.query.filter, seg, self.leaf_bitmaps(si, stream)).sum())
        return out

    def filtered_stats(self, stream=None):
        """(numDocsScanned, numEntriesScannedPostFilter) of a query with aggregation filters: per segment, the sum
        over that segment's swim lanes (filter_stats.lane_structure) of the lane's docs, and of docs x the columns the
        lane projects (FilteredAggregationOperator.java:96-98, FilteredGroupByOperator.java:159-161)."""
        from . import filter_stats as FS
        q = self.query
        docs = self.lane_docs(stream)
        scanned = post = 0
        for si, seg in enumerate(self.segs):
            w = int(docs[si, 0])
            for f, aggs in FS.lane_structure(q, seg):
                if f is None:
                    n = w
                elif isinstance(f, str):   # ("empty": the main filter matches nothing here)
                    n = 0
                else:
                    dev = self.lane_dev[self.lane_filters.index(f)]
                    n = w if dev == "all" else (0 if dev == "none" else int(docs[si, 1 + dev]))
                scanned += n
                post += n * FS.lane_projected_columns(q, aggs)
        return scanned, post

    def _presence_stride(self, i):
        """DISTINCTCOUNT presence bytes per group: the value count rounded up to 16 (PA_ACC_PRESENCE_U8)."""
        return (len(self.value_dicts[i]) + 15) & ~15

    def fetch_histograms(self, pi, num_groups, stream=None):
        """One ValueHistogram per fetched group (fetch_arrays' order) of value-histogram accumulator `pi`: the non-zero
        bins, compacted on the GPU (pa_query_fetch_histogram), as values of the table-wide value dictionary.
        Synchronises `stream`."""
        lib = L.lib()
        vd = np.asarray(self.value_dicts[pi], dtype=np.float64)
        n = int(num_groups)
        ends = np.zeros(max(n, 1), dtype=np.int64)
        total = L.check(lib.pa_query_fetch_histogram(self.handle, stream, pi, n, 0, ends.ctypes.data, None, None),
                        "pa_query_fetch_histogram")
        ids = OUTPUT_POOL.array("hist_ids", max(total, 1), np.int32)
        cnt = OUTPUT_POOL.array("hist_counts", max(total, 1), np.int64)
        if total:
            L.check(lib.pa_query_fetch_histogram(self.handle, stream, pi, n, total, ends.ctypes.data, ids.ctypes.data,
                                                 cnt.ctypes.data), "pa_query_fetch_histogram")
        values, counts = vd[ids[:total]], cnt[:total].copy()
        starts = np.concatenate([[0], ends[:n]])
        return [ValueHistogram(values[starts[g]:starts[g + 1]], counts[starts[g]:starts[g + 1]]) for g in range(n)]

    def percentiles(self, stream=None):
        """The final values of every PERCENTILE / PERCENTILEMV aggregation of the query for every fetched group, selected
        on the GPU without moving the bins (pa_query_percentiles: one rank select per group; the percentiles of one
        column share a pass) — the single-server and server-trim fast path. Returns (keys, {aggregation index:
        float64[groups]}) with keys as fetch_arrays gives them; a group without values gives -inf
        (PercentileAggregationFunction.DEFAULT_FINAL_RESULT). Synchronises `stream`."""
        lib = L.lib()
        q = self.query
        by_acc = {}
        for ai, (a, pi) in enumerate(zip(q.aggregations, self.agg_map)):
            if a.function in Q.PERCENTILE_FUNCTIONS:
                by_acc.setdefault(pi, []).append(ai)
        if self.handle is None or not by_acc:
            return np.zeros(0, dtype=np.int64), {ai: np.zeros(0) for ais in by_acc.values() for ai in ais}
        n = L.check(lib.pa_query_fetch(self.handle, stream, 0, None, None, None), "pa_query_fetch")
        n = max(n, 0 if q.group_by else 1)
        keys = np.zeros(max(n, 1), dtype=np.int64)
        counts = np.zeros(max(n, 1), dtype=np.int64)
        if n:
            L.check(lib.pa_query_fetch(self.handle, stream, n, keys.ctypes.data, counts.ctypes.data, None),
                    "pa_query_fetch")
        out = {}
        for pi, ais in by_acc.items():
            ps = np.array([q.aggregations[ai].percentile for ai in ais], dtype=np.float64)
            ids = np.full(max(n, 1) * len(ps), -1, dtype=np.int32)
            if n:
                L.check(lib.pa_query_percentiles(self.handle, stream, pi, n, len(ps), ps.ctypes.data, ids.ctypes.data),
                        "pa_query_percentiles")
            ids = ids[:n * len(ps)].reshape(n, len(ps))
            vd = np.asarray(self.value_dicts[pi], dtype=np.float64)
            for j, ai in enumerate(ais):
                col = ids[:, j]
                out[ai] = np.where(col >= 0, vd[np.maximum(col, 0)], -np.inf)
        return keys[:n], out

    def key_values(self, keys):
        """Keys -> one value array per group-by column (DictionaryBasedGroupKeyGenerator.getKeys). Direct key space:
        key = sum id_j * prod_{k<j} card_k. Hashed (pa_query_key_layout): component j at bit shift_j, a table-wide key
        id for dictionary columns, the value bits for raw ones (INT/FLOAT 32 bits, LONG/DOUBLE 64); two-word keys
        (keys of shape (n, 2)): component j in word shift_j // 64 at bit shift_j % 64."""
        if not self.hashed:
            return [gd[(keys // st) % len(gd)] for gd, st in zip(self.global_dicts, self.strides)]
        kk = np.asarray(keys, dtype=np.int64)
        words = [kk.view(np.uint64)] if kk.ndim == 1 else [np.ascontiguousarray(kk[:, w]).view(np.uint64)
                                                           for w in range(kk.shape[1])]
        out = []
        for gd, raw, shw in zip(self.global_dicts, self.raw_group_by, self.key_shifts):
            k, sh = words[shw // 64], shw % 64
            if gd is not None:
                bits = max(1, int(len(gd) - 1).bit_length())
            else:
                bits = 32 if raw in ("INT", "FLOAT") else 64
            comp = (k >> np.uint64(sh)) & np.uint64((1 << bits) - 1) if bits < 64 else (k >> np.uint64(sh))
            if gd is not None:
                out.append(gd[comp.astype(np.int64)])
            elif raw == "INT":
                out.append(comp.astype(np.uint32).view(np.int32))
            elif raw == "FLOAT":
                out.append(comp.astype(np.uint32).view(np.float32))
            elif raw == "LONG":
                out.append(comp.view(np.int64))
            else:
                out.append(comp.view(np.float64))
        return out

    def torch_device(self):
        """The GPU holding this executor's segments (GpuSegment(device=...)), else the current device."""
        import torch
        return torch.device("cuda", self.device if self.device is not None else torch.cuda.current_device())

    def leaf_bitmaps(self, segment_index, stream=None):
        """bool[leaves, num_docs]: every filter leaf (the engine's flattened leaf order) on every doc of one bound
        segment, computed on the GPU (pa_query_leaf_bitmaps). Synchronises `stream`."""
        import torch
        lib = L.lib()
        nl = int(self.spec.num_leaves)
        n = self.segs[segment_index].num_docs
        if nl == 0:
            return np.zeros((0, n), dtype=bool)
        words = L.check(lib.pa_query_leaf_bitmap_words(self.handle, segment_index), "pa_query_leaf_bitmap_words")
        dev = self.torch_device()
        buf = torch.zeros(nl * words, dtype=torch.int32, device=dev)
        L.check(lib.pa_query_leaf_bitmaps(self.handle, segment_index, buf.data_ptr(), stream), "pa_query_leaf_bitmaps")
        torch.cuda.synchronize(dev)  # (device-wide: covers `stream`)
        w = buf.cpu().numpy().view(np.uint8).reshape(nl, words * 4)
        return np.unpackbits(w, axis=1, bitorder="little")[:, :n].astype(bool)

    def fused_leap_counts(self, stream=None):
        """(E leaf, Z leaf, int64[segments, 3]) when the last scan counted the execution statistics of its two-leaf AND
        itself (the default where it applies; PA_QF_NO_FILTER_STATS turns it off. pa_query_leap_counts: per segment
        matched docs, leaps of AndDocIdIterator(A = Z, B = E), gave-up flag), else None. Synchronises `stream`."""
        lib = L.lib()
        if self.handle is None or not self.segs or not getattr(self, "_scanned", False):
            return None
        e = int(lib.pa_query_leap_leaf(self.handle))
        if e < 0:
            return None
        out = np.zeros((len(self.segs), 3), dtype=np.int64)
        L.check(lib.pa_query_leap_counts(self.handle, out.ctypes.data, stream), "pa_query_leap_counts")
        return e, 1 - e, out

    def execution_stats(self, stream=None, docs_total=None):
        """(numEntriesScannedInFilter, numEntriesScannedPostFilter) of this server's segments after the last scan: the
        reference's operator accounting counted by the library (pa_query_execution_stats) over the operator trees this
        host builds per segment (filter_stats.operator_trees = FilterOperatorUtils). Segments whose tree the engine
        does not express (filter_stats "device path") replay the iterators on the host over GPU leaf bitmaps;
        self.stats_replayed_segments counts them. docs_total: numDocsScanned of the scan (default: the last scan's own
        counter, so a call after execute() without a fetch is not stale)."""
        from . import filter_stats as FS
        self.stats_replayed_segments = self.stats_gpu_segments = 0
        if self.match_none or self.handle is None or not self.segs:
            return 0, 0  # EmptyFilterOperator: no entry read, no doc projected
        if getattr(self, "_stats_trees", None) is None:  # the operator trees of this prepared query, built once
            self._stats_trees = FS.operator_trees(self.query, self.segs, getattr(self, "leaf_params", None),
                                                  self.gsegs[0].column_ids)
        ops, roots, seg_tree = self._stats_trees
        out = np.zeros(3, dtype=np.int64)
        per = np.zeros(len(self.segs), dtype=np.int64)
        L.check(L.lib().pa_query_execution_stats(
            self.handle, len(ops), ops.ctypes.data, len(roots), roots.ctypes.data, seg_tree.ctypes.data,
            FS.projected_columns(self.query), -1 if docs_total is None else int(docs_total), out.ctypes.data,
            per.ctypes.data, stream), "pa_query_execution_stats")
        in_filter, post = int(out[0]), int(out[1])
        self.stats_gpu_segments = int(out[2])  # segments whose statistics took a GPU pass (not the scan's own counts)
        host = np.flatnonzero(per < 0).tolist()
        if host:
            self.stats_replayed_segments = len(host)
            hi, _ = FS.server_stats(self.query, [self.segs[i] for i in host],
                                    lambda i: self.leaf_bitmaps(host[i], stream))
            in_filter += hi
        return in_filter, post

    def fetch(self, stream=None, execution_stats=True, server_trim=False) -> IntermediateResult:
        """The results block of the last scan. Like the reference's results blocks (BaseResultsBlock.java:194) it carries
        the execution statistics — numEntriesScannedInFilter / PostFilter from pa_query_execution_stats, after the groups
        (execution_stats): execution_stats=False leaves them 0.
        server_trim=True: the block after the server's group trim, reduce.server_trim(self.fetch(...), query), with the
        kept groups chosen on the GPU and only their rows copied (pa_query_fetch_trimmed; trim.py). Shapes the device
        refuses take the full fetch and the host trim, so the answer is the same either way; self.last_trim =
        {"device": the GPU trimmed, "groups": non-empty groups, "kept": groups in the block}."""
        q = self.query
        if self.handle is None:
            self.last_trim = {"device": False, "groups": 0, "kept": 0}
            return self._empty_result()
        if server_trim:
            from . import reduce as R
            from . import trim as TR
            spec = None
            if q.group_by:
                try:
                    spec = TR.build_spec(TR.lower_order_by(q, self.agg_map, self.hashed), TR.trim_size(q))
                except TR.HostTrim:
                    pass
            arrays = None
            if spec is not None:
                try:
                    arrays = self.fetch_arrays(stream, pooled=True, trim_spec=spec)
                except L.PinotAmdError as e:
                    if getattr(e, "code", None) != L.PA_EUNSUPPORTED:
                        raise
            if arrays is None:
                full = self.fetch(stream, execution_stats)
                res = R.server_trim(full, q)
                self.last_trim = {"device": False, "groups": len(full.groups) if q.group_by else 1,
                                  "kept": len(res.groups) if q.group_by else 1}
                return res
            self.last_trim = {"device": True, "groups": self.trim_total_groups, "kept": len(arrays[0])}
            return self._result_from_arrays(arrays, stream, execution_stats)
        return self._result_from_arrays(self.fetch_arrays(stream, pooled=True), stream, execution_stats)

    def _result_from_arrays(self, arrays, stream, execution_stats):
        """fetch_arrays' columns (of every non-empty group, or of the trimmed ones) as the IntermediateResult."""
        lib = L.lib()
        q = self.query
        keys, counts, outs = arrays  # (converted to Python objects below)
        n = len(keys)
        res = IntermediateResult(list(q.aggregations), list(q.group_by))
        res.num_total_docs = sum(s.num_docs for s in self.all_segs)
        res.num_docs_scanned = int(lib.pa_query_matched_docs(self.handle))
        merged = getattr(self, "merged_stats", None)
        filtered = bool(self.lane_filters)
        if filtered and merged is not None and not isinstance(merged, str):
            raise L.PinotAmdError("a query with aggregation filters has no merged execution statistics")
        if filtered and merged is None:
            # numDocsScanned and numEntriesScannedPostFilter are sums over the swim lanes; numEntriesScannedInFilter is
            # not defined here: CombinedFilterOperator.java:62-67 turns the main filter into a bitmap through
            # BlockDocIdSet.toNonScanDocIdSet, whose scan is not counted (BlockDocIdSet.java:57-58)
            # (the lanes' per-segment docs came with fetch_arrays' own copy: no second synchronisation)
            res.num_docs_scanned, post = self.filtered_stats(stream)
            res.num_entries_scanned_in_filter = None
            res.num_entries_scanned_post_filter = post if execution_stats else 0
        elif filtered:
            # (summed across GPUs: the lanes' per-segment docs of the other ranks are not here)
            res.num_docs_scanned = None
            res.num_entries_scanned_in_filter = None
            if execution_stats:
                raise L.PinotAmdError("the merged block of a query with aggregation filters has no execution "
                                      "statistics: fetch(execution_stats=False)")
        elif merged is not None:
            # numDocsScanned was summed across GPUs (parallel.DistributedAccumulators.reduce): this rank's segments
            # cannot recount the statistics against it; the reduce summed every rank's own pair before its collective
            # (reduce(execution_stats=True), the default), or gathered none (NO_MERGED_STATS)
            if execution_stats:
                if isinstance(merged, str):  # (parallel.NO_MERGED_STATS)
                    raise L.PinotAmdError("the merged block has no execution statistics: reduce(execution_stats=True), "
                                          "or fetch(execution_stats=False)")
                res.num_entries_scanned_in_filter, res.num_entries_scanned_post_filter = merged
        elif execution_stats:
            res.num_entries_scanned_in_filter, res.num_entries_scanned_post_filter = self.execution_stats(
                stream, res.num_docs_scanned)
        key_cols = [kc.tolist() for kc in self.key_values(keys)]
        for j, e in enumerate(getattr(self, "group_by_expr", ())):
            if e >= 0 and self.programs[e].result_type == T.DOUBLE:
                # (one NaN key, -0.0 and 0.0 two: the reference's map compares doubleToLongBits)
                key_cols[j] = [T.DoubleKey(v) for v in key_cols[j]]
        cols = []  # one python list per query aggregation
        hists = {}
        moments = {}  # VAR / STDDEV / COVAR: one fetch per accumulator
        # FIRSTWITHTIME / LASTWITHTIME: one fetch per accumulator, over the union of its value columns + the time column
        time_rows = {}
        for a, pi in zip(q.aggregations, self.agg_map):
            if a.function in Q.WITH_TIME_FUNCTIONS:
                want = time_rows.setdefault(pi, [a.time_column])
                if a.column not in want:
                    want.append(a.column)
        for pi, want in list(time_rows.items()):
            segs_, _, vals_ = self.fetch_time_rows(pi, n, want, stream)
            time_rows[pi] = (segs_, vals_)
        lane_counts = self.fetch_lane_counts(n, stream) if self.dev_filters and not self.match_none else None
        group_counts = counts
        for ai, (a, pi) in enumerate(zip(q.aggregations, self.agg_map)):
            # the docs behind this aggregation: its lane's (a filtered aggregation) or the group's
            dev = self.lane_dev[self.agg_lane[ai]] if self.agg_lane[ai] >= 0 else "all"
            if dev == "none" or (self.match_none and filtered):
                cols.append([_empty_value(a) for _ in range(n)])  # a lane without docs
                continue
            counts = group_counts if dev == "all" else lane_counts[dev]
            if dev != "all" and a.function in ("MIN", "MAX", "MINMAXRANGE"):
                # a group its lane saw no doc of holds the accumulators' reset values: the functions' empty results
                seen = counts > 0
                for p_, empty in zip(pi if isinstance(pi, tuple) else (pi,),
                                     (np.inf, -np.inf) if a.function == "MINMAXRANGE" else
                                     ((np.inf,) if a.function == "MIN" else (-np.inf,))):
                    outs[p_] = np.where(seen, outs[p_], empty)
            if a.function == "COUNT":
                cols.append(counts.tolist())
            elif a.function == "AVG":
                cols.append([AvgPair(s_, c_) for s_, c_ in zip(outs[pi].tolist(), counts.tolist())])
            elif a.function == "AVGMV":
                cols.append([AvgPair(s_, int(c_)) for s_, c_ in zip(outs[pi[0]].tolist(), outs[pi[1]].tolist())])
            elif a.function == "COUNTMV":
                cols.append([int(v) for v in outs[pi].tolist()])
            elif a.function in Q.HLL_FUNCTIONS:
                log2m = self.pa_aggs[pi][2]
                regs = outs[pi].reshape(n, 1 << log2m)
                cols.append([HyperLogLog(log2m, regs[r]) for r in range(n)])
            elif a.function in ("MINMAXRANGE", "MINMAXRANGEMV"):
                cols.append([MinMaxRangePair(lo, hi) for lo, hi in zip(outs[pi[0]].tolist(), outs[pi[1]].tolist())])
            elif a.function in Q.PERCENTILE_FUNCTIONS:
                # the DoubleArrayList of Percentile(MV)AggregationFunction as a multiset; aggregations of one column
                # share the accumulator, so its groups are fetched once
                if pi not in hists:
                    hists[pi] = self.fetch_histograms(pi, n, stream)
                cols.append(hists[pi])
            elif a.function in Q.MOMENT_FUNCTIONS:
                if pi not in moments:
                    moments[pi] = self.fetch_moments(pi, n, stream)
                cols.append(moments[pi])
            elif a.function in Q.WITH_TIME_FUNCTIONS:
                segs_, vals_ = time_rows[pi]
                stored = self.with_time_stored[a.column]  # (from the plan: a placeholder plan leaves no segment here)
                cols.append([with_time_default(a.function, a.data_type) if segs_[r] < 0 else
                             ValueTimePair(java_cast(vals_[a.column][r], stored, a.data_type), int(vals_[a.time_column][r]))
                             for r in range(n)])
            elif a.function in Q.DISTINCT_SET_FUNCTIONS:
                # the value set of BaseDistinctAggregateAggregationFunction (DISTINCTCOUNT / DISTINCTSUM / DISTINCTAVG)
                vd = self.value_dicts[pi]
                pres = outs[pi].reshape(n, self._presence_stride(pi))[:, :len(vd)]
                if a.function in Q.BITMAP_FUNCTIONS:  # (DISTINCTCOUNTBITMAP: the values' Java hash codes)
                    dt = self.segs[0].column(a.column).data_type
                    hc = np.array([java_hash_code(v, dt) for v in vd.tolist()], dtype=np.int64)
                    cols.append([set(hc[np.flatnonzero(pres[r])].tolist()) for r in range(n)])
                else:
                    cols.append([set(vd[np.flatnonzero(pres[r])].tolist()) for r in range(n)])
            else:
                cols.append(outs[pi].tolist())
        rows = list(zip(*cols)) if cols else [()] * n
        if q.group_by:
            res.groups = {tuple(kc[r] for kc in key_cols): list(rows[r]) for r in range(n)}
            # GroupByOperator.java:112 per segment, OR-ed by GroupByCombineOperator.java:154
            res.num_groups_limit_reached = int(L.lib().pa_query_num_groups_limit_reached(self.handle)) > 0
        else:
            res.row = list(rows[0])
        return res

    def _empty_result(self):
        """The results block of a segment set without docs: no groups, or the aggregation functions' empty
        intermediate results (COUNT 0, SUM 0.0, MIN +inf, MAX -inf, AVG (0.0, 0), empty HLL / value set)."""
        q = self.query
        res = IntermediateResult(list(q.aggregations), list(q.group_by))
        if not q.group_by:
            res.row = [_empty_value(a) for a in q.aggregations]
        return res

    def run(self, stream=None) -> IntermediateResult:
        self.execute(stream)
        return self.fetch(stream)

    def close(self):
        if self.handle:
            L.lib().pa_query_destroy(self.handle)
            self.handle = None
        if self.placeholder is not None:
            self.placeholder.close()
            self.placeholder = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# the kernel variant behind each pa_query_plan strategy code (pa_device.h Strategy)
STRATEGY_VARIANTS = {0: "lds", 1: "global", 2: "partitioned", 4: "lane", 5: "lane_cnt", 6: "lane_raw", 7: "lane_dict",
                     8: "gdense4", 9: "gdense8", 10: "gdense12", 11: "gdense_rs12", 12: "gdense_rs8", 14: "gdense_lm8",
                     15: "gdense_lm16", 128: "select", 129: "distinct_lds", 130: "distinct_global",
                     131: "filtered_lds", 132: "filtered_global", 133: "expr_lds", 134: "expr_global",
                     135: "time_rows_lds", 136: "time_rows_global", 137: "moments_lds", 138: "moments_global"}
TIME_ROW_AGGS = (L.PA_AGG_LAST_ROW_BY_TIME, L.PA_AGG_FIRST_ROW_BY_TIME)


class SelectionExecutor(GpuQueryExecutor):
    """SELECT columns | * ... [WHERE ...] [ORDER BY c1 [DESC], ...] LIMIT [offset,] n over the segments of one GPU:
    SelectionOnlyOperator / SelectionOrderByOperator on every segment + SelectionOrderByCombineOperator, as one fused
    filter + top-K scan (include/pinot_amd.h "selection queries"). The server keeps K = offset + limit rows
    (SelectionOrderByOperator._numRowsToKeep); reduce.merge_selection applies the offset.

    table_dicts: optional {ORDER BY column: values ascending in the column's order (selection.table_order_dictionary)}
    — the table-wide dictionary whose ranks the sort keys hold; ranks of different servers agree only when they share
    it. By default the union of these segments' dictionaries."""

    def __init__(self, query: Q.Query, gpu_segments: List[GpuSegment], flags=0, table_dicts=None, tuning=None):
        from . import selection as S
        if not query.is_selection:
            raise ValueError("not a selection query")
        if not gpu_segments:
            raise ValueError("no segments")
        if str(query.options.get("enableNullHandling", "false")).lower() == "true":
            raise UnsupportedQuery("selection with null handling")
        self.selection = query
        self.num_rows = int(query.offset) + int(query.limit)
        if self.num_rows > L.PA_MAX_SELECT_ROWS:
            raise UnsupportedQuery("selection keeps %d rows (offset + limit), more than PA_MAX_SELECT_ROWS (%d)"
                                   % (self.num_rows, L.PA_MAX_SELECT_ROWS))
        seg0 = gpu_segments[0].segment
        for o in query.order_by:
            if not isinstance(o.expr, str) or o.expr not in seg0.columns:
                raise UnsupportedQuery("selection ordered by a transform expression: %r" % (o.expr,))
        for c in query.select_columns:
            if c not in seg0.columns:
                raise UnsupportedQuery("transform expression or unknown column in the select list: %r" % (c,))
        if len(query.order_by) > L.PA_MAX_ORDER_BY:
            raise UnsupportedQuery("too many order-by columns")
        self.result_columns = S.result_columns(query, seg0.columns)
        if len(self.result_columns) > L.PA_MAX_SELECT_COLUMNS:
            raise UnsupportedQuery("too many select columns")
        for c in self.result_columns:
            if not seg0.column(c).single_value:
                raise UnsupportedQuery("multi-value column %s in a selection" % c)
        self.result_types = [seg0.column(c).data_type for c in self.result_columns]
        self.order_columns = []
        for o in query.order_by:
            if o.expr not in [c for c, _ in self.order_columns]:
                self.order_columns.append((o.expr, bool(o.asc)))
        self.order_dicts = dict(table_dicts or {})
        self.total_docs = sum(g.segment.num_docs for g in gpu_segments)
        # the reference runs SelectionOrderByOperator (a full scan whose statistics are modelled) only when the first
        # ORDER BY column is not sorted in the segment; otherwise, and without ORDER BY, it stops early
        bound = [g.segment for g in gpu_segments if g.segment.num_docs > 0]
        self.stats_modelled = bool(self.order_columns) and not any(
            s.column(self.order_columns[0][0]).is_sorted for s in bound)
        self.bound_index = [i for i, g in enumerate(gpu_segments) if g.segment.num_docs > 0]
        count = dataclasses.replace(query, aggregations=[Q.Aggregation("COUNT")], aliases=[None], order_by=[],
                                    select_columns=[], num_select_aggs=1, select_star=False, limit=10, offset=0)
        if self.num_rows == 0 or not bound:  # EmptySelectionOperator / nothing to scan: no plan, no launch
            self.query, self.handle, self.placeholder, self.segs, self.gsegs = count, None, None, [], []
            self.all_segs = [g.segment for g in gpu_segments]
            self.match_none = False
            return
        try:
            super().__init__(count, gpu_segments, flags=flags, tuning=tuning)
        except L.PinotAmdError as e:
            if "(%d)" % -4 in str(e) and not isinstance(e, UnsupportedQuery):  # PA_EUNSUPPORTED
                raise UnsupportedQuery(str(e))
            raise

    def _after_create(self):
        from . import selection as S
        ids = self.gsegs[0].column_ids
        spec = L.SelectSpec()
        spec.num_order_by = len(self.order_columns)
        self.order_remaps = []  # [order-by][segment] -> int32 ranks, or None for identity / a raw column
        for j, (name, asc) in enumerate(self.order_columns):
            cols = [s.column(name) for s in self.segs]
            spec.order_by_columns[j] = ids[name]
            spec.order_by_desc[j] = 0 if asc else 1
            if not any(c.has_dictionary for c in cols):
                spec.order_by_cardinality[j] = 0  # raw: ordered by value
                self.order_remaps.append([None] * len(cols))
                continue
            if not all(c.has_dictionary for c in cols):
                raise UnsupportedQuery("order-by column %s is dictionary-encoded in some segments only" % name)
            dt = cols[0].data_type
            if name in self.order_dicts:
                keys = S.order_keys(self.order_dicts[name], dt)
            else:
                _, keys = S.table_order_dictionary([c.dictionary for c in cols], dt)
            spec.order_by_cardinality[j] = len(keys)
            rms = []
            for c in cols:
                rm = S.order_remap(keys, c.dictionary, dt)
                rms.append(None if len(rm) == len(keys) and np.array_equal(rm, np.arange(len(keys))) else rm)
            self.order_remaps.append(rms)
        spec.num_columns = len(self.result_columns)
        for c, name in enumerate(self.result_columns):
            spec.columns[c] = ids[name]
        spec.num_rows = self.num_rows
        L.check(L.lib().pa_query_set_selection(self.handle, ctypes.byref(spec)), "pa_query_set_selection")

    def _before_prepare(self):
        for j, rms in enumerate(self.order_remaps):
            for si, rm in enumerate(rms):
                if rm is not None:
                    self._keep.append(rm)
                    L.check(L.lib().pa_query_bind_order_remap(self.handle, si, j, rm.ctypes.data),
                            "pa_query_bind_order_remap")

    def counters(self):
        """{candidates appended, compactions, scan waves, CAP} of the scan the last fetch read."""
        out = np.zeros(4, dtype=np.int64)
        L.check(L.lib().pa_query_selection_counters(self.handle, out.ctypes.data), "pa_query_selection_counters")
        return dict(zip(("appended", "compactions", "waves", "cap"), out.tolist()))

    def fetch(self, stream=None, execution_stats=True):
        """The SelectionResult of the last scan (synchronises `stream`)."""
        from . import selection as S
        res = S.SelectionResult(list(self.result_columns), list(self.result_types), num_total_docs=self.total_docs)
        if self.handle is None:  # LIMIT 0 (EmptySelectionOperator: statistics 0, 0, 0) or no docs at all
            res.num_docs_scanned = res.num_entries_scanned_in_filter = res.num_entries_scanned_post_filter = 0
            return res
        lib = L.lib()
        K, nout = self.num_rows, len(self.result_columns)
        segs, docs = np.zeros(K, dtype=np.int32), np.zeros(K, dtype=np.int32)
        keys = np.zeros(K, dtype=np.uint64)
        cells = np.zeros((max(nout, 1), K), dtype=np.int64)
        ptrs = (ctypes.c_void_p * max(nout, 1))(*[cells[c].ctypes.data for c in range(max(nout, 1))])
        n = L.check(lib.pa_query_fetch_selection(self.handle, stream, K, segs.ctypes.data, docs.ctypes.data,
                                                 keys.ctypes.data, ptrs), "pa_query_fetch_selection")
        segs, docs, keys = segs[:n], docs[:n], keys[:n]
        cols = []
        for c, name in enumerate(self.result_columns):
            out = np.empty(n, dtype=object)
            for si in np.unique(segs).tolist():
                m = segs == si
                col = self.segs[si].column(name)
                cell = cells[c, :n][m]
                if col.has_dictionary:
                    vals = col.dictionary[cell]
                elif col.data_type in ("FLOAT", "DOUBLE"):
                    vals = cell.view(np.float64).astype(np.float32 if col.data_type == "FLOAT" else np.float64)
                else:
                    vals = cell.astype(np.int32 if col.data_type == "INT" else np.int64)
                out[m] = vals.tolist()
            cols.append(out.tolist())
        res.rows = [list(r) for r in zip(*cols)] if cols else [[] for _ in range(n)]
        res.segments = np.asarray([self.bound_index[s] for s in segs.tolist()], dtype=np.int32)
        res.docs, res.keys = docs.copy(), keys.copy()
        if self.stats_modelled:
            matched = int(lib.pa_query_matched_docs(self.handle))
            res.num_docs_scanned = matched
            per = np.zeros(len(self.segs), dtype=np.int64)
            L.check(lib.pa_query_selection_segment_docs(self.handle, per.ctypes.data), "pa_query_selection_segment_docs")
            res.num_entries_scanned_post_filter = S.post_filter_entries(
                per.tolist(), K, len(self.order_columns), nout - len(self.order_columns))
            if execution_stats:
                res.num_entries_scanned_in_filter = self.execution_stats(stream, matched)[0]
        return res

    def run(self, stream=None):
        if self.handle is not None:
            self.execute(stream)
        return self.fetch(stream)


class DistinctExecutor(GpuQueryExecutor):
    """SELECT DISTINCT c1, c2, ... [WHERE ...] [ORDER BY ci [DESC], ...] [LIMIT n] over the segments of one GPU:
    DistinctOperator on every segment + DistinctCombineOperator, as one fused filter + key-presence bitmap scan and a
    rank pass over the bits (include/pinot_amd.h "distinct queries"). The rows come back under the completed order
    (distinct.completed_order), so which records a limit keeps is a function of the data.

    table_dicts: optional {DISTINCT column: values ascending in the column's order (selection.table_order_dictionary)}
    — the table-wide dictionary whose ids the keys hold; by default the union of these segments' dictionaries.
    force_scan: run the GPU scan even where the reference answers from the dictionary (one dictionary column, no
    filter); the rows are the same."""

    def __init__(self, query: Q.Query, gpu_segments: List[GpuSegment], flags=0, table_dicts=None, tuning=None,
                 force_scan=False):
        from . import distinct as D
        from . import selection as S
        if not query.is_distinct:
            raise ValueError("not a distinct query")
        if not gpu_segments:
            raise ValueError("no segments")
        if str(query.options.get("enableNullHandling", "false")).lower() == "true":
            raise UnsupportedQuery("distinct with null handling")
        self.distinct = query
        self.result_columns = list(query.select_columns)
        if len(set(self.result_columns)) != len(self.result_columns):
            raise UnsupportedQuery("a column appears twice in the DISTINCT list")
        if len(self.result_columns) > L.PA_MAX_GROUP_BY:
            raise UnsupportedQuery("too many DISTINCT columns")
        seg0 = gpu_segments[0].segment
        for c in self.result_columns:
            if c not in seg0.columns:
                raise UnsupportedQuery("transform expression or unknown column in the DISTINCT list: %r" % (c,))
        self.result_types = [seg0.column(c).data_type for c in self.result_columns]
        self.order = D.completed_order(query)
        self.total_docs = sum(g.segment.num_docs for g in gpu_segments)
        bound = [g.segment for g in gpu_segments if g.segment.num_docs > 0]
        # table-wide dictionaries in the reference's value order (STRING: UTF-16 code units, not numpy's code points)
        dicts = dict(table_dicts or {})
        for c, dt in zip(self.result_columns, self.result_types):
            if c not in dicts and bound and all(s.column(c).has_dictionary for s in bound):
                ds = [s.column(c).dictionary for s in bound]
                if dt == "STRING" or any(d is not ds[0] and not (len(d) == len(ds[0]) and np.array_equal(d, ds[0]))
                                         for d in ds):
                    dicts[c] = S.table_order_dictionary(ds, dt)[0]
        self.fast_path = bool(bound) and not force_scan and D.dictionary_fast_path(query, [g.segment for g in gpu_segments])
        group = dataclasses.replace(query, aggregations=[], aliases=[], group_by=list(self.result_columns), order_by=[],
                                    select_columns=[], num_select_aggs=0, distinct=False, limit=10, offset=0)
        if not bound or self.fast_path:  # nothing to scan, or answered from the dictionary: no plan, no launch
            self.query, self.handle, self.placeholder, self.segs, self.gsegs = group, None, None, bound, []
            self.all_segs = [g.segment for g in gpu_segments]
            self.match_none = False
            self.table_dicts = dicts
            return
        try:
            super().__init__(group, gpu_segments, flags=flags, enforce_num_groups_limit=False, table_dicts=dicts,
                             tuning=tuning)
        except L.PinotAmdError as e:
            if "(%d)" % -4 in str(e) and not isinstance(e, UnsupportedQuery):  # PA_EUNSUPPORTED
                raise UnsupportedQuery(str(e))
            raise

    def _group_remap(self, name, table_dict, dictionary):
        from . import selection as S
        dt = self.result_types[self.result_columns.index(name)]
        return S.order_remap(S.order_keys(table_dict, dt), dictionary, dt)

    def _after_create(self):
        spec = L.DistinctSpec()
        named = [(j, asc) for j, asc in self.order[:len({o.expr for o in self.distinct.order_by})]]
        spec.num_order_by = len(named)
        for i, (j, asc) in enumerate(named):
            spec.order_by_index[i] = j
            spec.order_by_desc[i] = 0 if asc else 1
        spec.limit = int(self.distinct.limit)
        L.check(L.lib().pa_query_set_distinct(self.handle, ctypes.byref(spec)), "pa_query_set_distinct")

    def fetch(self, stream=None, execution_stats=True):
        """The DistinctResult of the last scan (synchronises `stream`)."""
        from . import distinct as D
        q = self.distinct
        if self.fast_path:
            return D.dictionary_distinct(q, self.all_segs)
        res = D.DistinctResult(list(self.result_columns), list(self.result_types), num_total_docs=self.total_docs)
        if self.handle is None or self.match_none:  # no docs at all / EmptyFilterOperator: nothing read
            res.num_docs_scanned = res.num_entries_scanned_in_filter = res.num_entries_scanned_post_filter = 0
            return res
        lib = L.lib()
        ncol = len(self.result_columns)
        present = ctypes.c_int64()
        cap = min(int(q.limit), self.num_keys, sum(s.num_docs for s in self.segs))
        if cap > 1 << 20:  # a capacity-0 call only counts, so the rows are copied once, at the exact size
            cap = L.check(lib.pa_query_fetch_distinct(self.handle, stream, 0, None, ctypes.byref(present)),
                          "pa_query_fetch_distinct")
        ids = OUTPUT_POOL.array("distinct_ids", max(1, cap * ncol), np.int32)
        n = L.check(lib.pa_query_fetch_distinct(self.handle, stream, cap, ids.ctypes.data, ctypes.byref(present)),
                    "pa_query_fetch_distinct")
        n = min(n, cap)
        ids = ids[:n * ncol].reshape(n, ncol)
        cols = [np.asarray(self.global_dicts[j])[ids[:, j]].tolist() for j in range(ncol)]
        res.rows = [list(r) for r in zip(*cols)]
        res.present = int(present.value)
        # exact with ORDER BY (every matching doc is offered), or when the limit was not reached (no early termination)
        if q.order_by or res.present < int(q.limit):
            matched = int(lib.pa_query_matched_docs(self.handle))
            res.num_docs_scanned = matched
            res.num_entries_scanned_post_filter = matched * ncol
            if execution_stats:
                res.num_entries_scanned_in_filter = self.execution_stats(stream, matched)[0]
        return res

    def execute(self, stream=None):
        if self.handle is not None:
            super().execute(stream)

    def run(self, stream=None):
        self.execute(stream)
        return self.fetch(stream)


def _empty_value(a):
    """An aggregation function's intermediate result over no docs."""
    fn = Q.base_function(a.function)
    if fn in Q.WITH_TIME_FUNCTIONS:
        return with_time_default(fn, a.data_type)
    if fn in Q.VARIANCE_FUNCTIONS:  # (extractAggregationResult of an empty holder)
        return VarianceTuple(0, 0.0, 0.0)
    if fn in Q.COVARIANCE_FUNCTIONS:
        return CovarianceTuple(0.0, 0.0, 0.0, 0)
    return ({"COUNT": 0, "SUM": 0.0, "MIN": float("inf"), "MAX": float("-inf")}.get(fn) if fn in
            ("COUNT", "SUM", "MIN", "MAX") else
            AvgPair(0.0, 0) if fn == "AVG" else
            HyperLogLog(a.log2m) if fn in ("DISTINCTCOUNTHLL", "DISTINCTCOUNTRAWHLL") else
            MinMaxRangePair(float("inf"), float("-inf")) if fn == "MINMAXRANGE" else
            ValueHistogram() if fn == "PERCENTILE" else set())


def _fold_constants(f):
    """A filter tree with its TRUE / FALSE literals folded away (AND / OR / NOT over constants, as FilterPlanNode folds
    MatchAll / Empty operators): a BoolFilter when the whole tree is constant."""
    if isinstance(f, (Q.And, Q.Or)):
        is_and = isinstance(f, Q.And)
        kids = []
        for c in (_fold_constants(c) for c in f.children):
            if isinstance(c, Q.BoolFilter):
                if c.value != is_and:   # FALSE in an AND, TRUE in an OR: the whole node
                    return c
                continue
            kids.append(c)
        if not kids:
            return Q.BoolFilter(is_and)
        return kids[0] if len(kids) == 1 else type(f)(tuple(kids))
    if isinstance(f, Q.Not):
        c = _fold_constants(f.child)
        return Q.BoolFilter(not c.value) if isinstance(c, Q.BoolFilter) else Q.Not(c)
    return f


def _has_comparison(f):
    if isinstance(f, (Q.And, Q.Or)):
        return any(_has_comparison(c) for c in f.children)
    if isinstance(f, Q.Not):
        return _has_comparison(f.child)
    return isinstance(f, Q.Comparison)


def _py(v):
    if isinstance(v, np.generic):
        return v.item()
    return v
