"""Server-side group trim on the GPU: the lowering of ORDER BY ... LIMIT over GROUP BY to pa_query_fetch_trimmed.

reduce.server_trim (IndexedTable.finish / TableResizer.resizeRecordsMap) sorts every group with a comparator and keeps
the first `trim`. The device restates the comparator as a string of unsigned 64-bit order words per group, most
significant first, and selects the `trim` smallest strings:

  group-by column     its table-wide id (the table dictionaries are sorted ascending: id order is value order)
  COUNT               the 64-bit count
  SUM / MIN / MAX     the aggregation's final double (a 96-bit sum rounded once: sums that round to one double tie),
                      -0.0 mapped to +0.0, then the order-preserving transform of the bits
  AVG                 sum / count, MINMAXRANGE max - min, in IEEE double, encoded the same way
  DESC                the word complemented
  tie word (last)     the key with group-by column 0 most significant: sum digit_j * prod_{k>j} card_k (unique)

Without ORDER BY the string is the tie word alone. NaN term values are out of scope: the host comparator is no total
order over them. lower_order_by raises HostTrim for the shapes the device refuses (the engine then trims the full fetch
with reduce.server_trim); reference_trim is the numpy restatement of the words, for the tests.
"""
import numpy as np

from . import _lib as L
from . import query as Q

MAX_TERMS = L.PA_MAX_TRIM_TERMS


class HostTrim(Exception):
    """The query's trim runs on the host (reduce.server_trim over the full fetch); str(e) says why."""


def trim_size(query):
    """Groups a server keeps: GroupByUtils.getTableCapacity under ORDER BY, else the limit (reduce.server_trim)."""
    if query.order_by:
        return max(query.limit * 5, query.min_server_group_trim_size)
    return query.limit


def lower_order_by(query, agg_map, hashed=False):
    """query.order_by -> [(kind, index, index2, desc)] over the executor's accumulators (agg_map: per query aggregation
    its accumulator index, or the pair of them). Raises HostTrim for a shape the device refuses."""
    if hashed or any(isinstance(g, Q.Expr) for g in query.group_by):
        raise HostTrim("hashed key space")
    for a in query.aggregations:
        if a.filter is not None:
            raise HostTrim("the query has aggregation filters")
        if a.function in Q.PERCENTILE_FUNCTIONS:
            raise HostTrim("the query has a PERCENTILE aggregation (value histogram)")
        if a.function in Q.MOMENT_FUNCTIONS:
            raise HostTrim("the query has a VAR / STDDEV / COVAR aggregation (moment sums)")
    if len(query.order_by) > MAX_TERMS:
        raise HostTrim("more than %d ORDER BY terms" % MAX_TERMS)
    terms = []
    for ob in query.order_by:
        desc = 0 if ob.asc else 1
        if not isinstance(ob.expr, Q.Aggregation):
            terms.append((L.PA_TRIM_KEY_COLUMN, query.group_by.index(ob.expr), 0, desc))
            continue
        idx = None
        for i, a in enumerate(query.aggregations):  # (the last match, as reduce._order_key_fn)
            if a == ob.expr:
                idx = i
        if idx is None:
            raise ValueError("ORDER BY aggregation not in select list: %r" % (ob.expr,))
        fn, pi = ob.expr.function, agg_map[idx]
        if fn == "COUNT":
            terms.append((L.PA_TRIM_COUNT, 0, 0, desc))
        elif fn in ("SUM", "SUMMV", "MIN", "MINMV", "MAX", "MAXMV"):
            terms.append((L.PA_TRIM_AGG, int(pi), 0, desc))
        elif fn == "AVG":
            terms.append((L.PA_TRIM_AVG, int(pi), 0, desc))
        elif fn in ("MINMAXRANGE", "MINMAXRANGEMV"):
            terms.append((L.PA_TRIM_RANGE, int(pi[1]), int(pi[0]), desc))  # (agg_map: (MIN, MAX))
        else:
            raise HostTrim("ORDER BY %s" % fn)
    return terms


def build_spec(terms, trim):
    spec = L.TrimSpec()
    spec.num_terms = len(terms)
    for e, (kind, index, index2, desc) in enumerate(terms):
        spec.kind[e], spec.index[e], spec.index2[e], spec.desc[e] = kind, index, index2, desc
    spec.trim = int(trim)
    return spec


def double_word(v):
    """float64[n] -> uint64[n] of the same order, -0.0 tying with +0.0."""
    v = np.array(v, dtype=np.float64)
    v[v == 0] = 0.0
    b = v.view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))


def order_words(keys, cards, counts, finals, terms):
    """The word columns of the module docstring, most significant first (the tie word last), as uint64 arrays."""
    keys = np.asarray(keys, dtype=np.int64)
    counts = np.asarray(counts, dtype=np.int64)
    digits, rem = [], keys.copy()
    for c in cards:
        digits.append(rem % int(c))
        rem = rem // int(c)
    words = []
    for kind, index, index2, desc in terms:
        if kind == L.PA_TRIM_KEY_COLUMN:
            w = digits[index].astype(np.uint64)
        elif kind == L.PA_TRIM_COUNT:
            w = counts.astype(np.uint64)
        elif kind == L.PA_TRIM_AGG:
            w = double_word(finals[index])
        elif kind == L.PA_TRIM_AVG:
            w = double_word(np.asarray(finals[index], dtype=np.float64) / counts.astype(np.float64))
        elif kind == L.PA_TRIM_RANGE:
            w = double_word(np.asarray(finals[index], dtype=np.float64) - np.asarray(finals[index2], dtype=np.float64))
        else:
            raise ValueError("term kind %r" % (kind,))
        words.append(~w if desc else w)
    tie = np.zeros(len(keys), dtype=np.uint64)
    for d, c in zip(digits, cards):
        tie = tie * np.uint64(int(c)) + d.astype(np.uint64)
    words.append(tie)
    return words


def reference_trim(keys, cards, counts, finals, terms, trim):
    """Positions (ascending) of the `trim` groups the device keeps: keys int64[n] of the direct key space with
    cardinalities `cards` (digit j of a key has weight prod_{k<j} card_k), counts int64[n], finals one float64[n] per
    accumulator, terms as lower_order_by gives them."""
    n = len(keys)
    if n <= trim:
        return np.arange(n)
    words = order_words(keys, cards, counts, finals, terms)
    order = np.lexsort(tuple(reversed(words)))  # (lexsort: the last key is the primary one)
    return np.sort(order[:max(int(trim), 0)])
