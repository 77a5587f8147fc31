"""Restatement of the reference's distinct query (SELECT DISTINCT c1, c2, ... [WHERE] [ORDER BY] [LIMIT]) over a list
of segments: the checker of tests/test_distinct.py and tests/test_gpu_distinct.py. It uses the product only for
parse_sql's Query and the Segment model; the filter (selection_ref.filter_mask), the executors, the dictionary operator,
the table merge, the reducer and the statistics are written out here on their own.

  DistinctPlanNode.java:50-78                   which operator runs (uses_dictionary_operator)
  DictionaryBasedDistinctOperator.java:56-133   dictionary_operator
  DistinctOperator.java:55-84                   distinct_operator: blocks of 10000 docs (DocIdSetPlanNode.
                                                MAX_DOC_PER_CALL) offered to the executor until it is satisfied
  DictionaryBasedMultiColumnDistinctOnlyExecutor.java:44-84,
  DictionaryBasedSingleColumnDistinctOnlyExecutor    distinct_only: a set that stops at `limit` records, first seen in
                                                docId order
  DictionaryBasedMultiColumnDistinctOrderByExecutor.java:55-121,
  DictionaryBasedSingleColumnDistinctOrderByExecutor distinct_order_by: a set and a bounded heap ordered by the ORDER BY
                                                columns' dictIds; a record replaces the heap's worst only when strictly
                                                better
  DistinctTable.java:213-280                    merge_tables (addWithoutOrderBy / addWithOrderBy)
  DistinctDataTableReducer.java:56,122          reduce: the limit alone, rows sorted when ORDER BY is present

Two answers of the reference are not functions of the data: which `limit` records survive without ORDER BY (the combine
merges in completion order) and which records of the tie class at the cut survive an ORDER BY on a subset of the
columns. `reference_*` below follow the reference literally for a given segment order (what the golden cases pin:
sizes and sets); `completed_*` is the deterministic completion the engine implements: the ORDER BY entries, then the
remaining DISTINCT columns ascending in select order."""
import functools
import heapq

import numpy as np

import selection_ref as SR

BLOCK_DOCS = 10000  # DocIdSetPlanNode.MAX_DOC_PER_CALL


def order_entries(query):
    """[(column index, ascending)] of the ORDER BY clause as written (each column once)."""
    cols = list(query.select_columns)
    out = []
    for o in query.order_by:
        j = cols.index(o.expr)
        if j not in [x for x, _ in out]:
            out.append((j, bool(o.asc)))
    return out


def completed_entries(query):
    named = [j for j, _ in order_entries(query)]
    return order_entries(query) + [(j, True) for j in range(len(query.select_columns)) if j not in named]


def column_types(query, segments):
    seg = next(s for s in segments if s.num_docs)
    return [seg.column(c).data_type for c in query.select_columns]


def _rank_columns(records, types):
    """int64[len(records), columns]: every component's dense rank in its column's order (selection_ref.value_ranks)."""
    if not records:
        return np.zeros((0, len(types)), dtype=np.int64)
    return np.stack([SR.value_ranks(np.array([r[j] for r in records], dtype=object if t == "STRING" else None), t)
                     for j, t in enumerate(types)], axis=1)


def sort_records(records, types, entries):
    """Records sorted by `entries` (most significant first) with numpy.lexsort over the columns' value ranks."""
    if not records:
        return []
    ranks = _rank_columns(records, types)
    keys = [ranks[:, j] if asc else -ranks[:, j] for j, asc in reversed(entries)]
    return [records[i] for i in np.lexsort(keys).tolist()]


def _ident(v, t):
    return SR._float_id(v) if t in ("FLOAT", "DOUBLE") else v


def unique_records(records, types):
    seen, out = set(), []
    for r in records:
        k = tuple(_ident(v, t) for v, t in zip(r, types))
        if k not in seen:
            seen.add(k)
            out.append(list(r))
    return out


def matching_records(query, seg):
    """The value records of the docs of one segment that pass the filter, in docId order."""
    if not seg.num_docs:
        return []
    docs = np.flatnonzero(SR.filter_mask(query.filter, seg))
    cols = [SR.decoded(seg, c)[docs].tolist() for c in query.select_columns]
    return [list(r) for r in zip(*cols)]


# ------------------------------------------------------------------ executors (one doc at a time, docId order)
def distinct_only(records, types, limit):
    """DistinctOnly executors: (records kept in first-seen order, docs processed). Whole blocks of BLOCK_DOCS matching
    docs are processed; the executor stops adding at `limit` and the operator stops after the block that satisfied it."""
    kept, seen, processed = [], set(), 0
    for b0 in range(0, len(records), BLOCK_DOCS):
        block = records[b0:b0 + BLOCK_DOCS]
        processed += len(block)
        for r in block:
            k = tuple(_ident(v, t) for v, t in zip(r, types))
            if k not in seen:
                seen.add(k)
                kept.append(list(r))
                if len(kept) >= limit:
                    break
        if len(kept) >= limit:
            break
    return kept, processed


def distinct_order_by(records, types, entries, limit):
    """DistinctOrderBy executors: a set + a heap of `limit` records whose top is the worst under the ORDER BY entries; a
    new record enters a full heap only when strictly better than the worst. Returns (records kept, docs processed)."""
    ranks = _rank_columns(records, types)

    def okey(i):
        return tuple(int(ranks[i, j]) if asc else -int(ranks[i, j]) for j, asc in entries)

    seen, heap = set(), []  # heap of (negated order key wrapper) -> implemented as a max-heap through sort keys
    for i, r in enumerate(records):
        k = tuple(_ident(v, t) for v, t in zip(r, types))
        if k in seen:
            continue
        ok = okey(i)
        if len(heap) < limit:
            seen.add(k)
            heapq.heappush(heap, (_Neg(ok), i, k))
        elif limit and ok < heap[0][0].key:
            seen.discard(heap[0][2])
            seen.add(k)
            heapq.heapreplace(heap, (_Neg(ok), i, k))
    return [list(records[i]) for _, i, _ in heap], len(records)


@functools.total_ordering
class _Neg:
    """Reverses the order of a key (heapq is a min-heap; the executor's heap keeps the worst record on top)."""

    def __init__(self, key):
        self.key = key

    def __eq__(self, other):
        return self.key == other.key

    def __lt__(self, other):
        return self.key > other.key


# ------------------------------------------------------------------ operators
def uses_dictionary_operator(query, seg):
    return (len(query.select_columns) == 1 and query.filter is None and
            seg.column(query.select_columns[0]).has_dictionary)


def dictionary_operator(query, seg):
    """(records, statistics (numDocsScanned, inFilter, postFilter, totalDocs)): the first / last n dictionary values."""
    col = seg.column(query.select_columns[0])
    t = col.data_type
    vals = np.asarray(col.dictionary).tolist()
    vals = [vals[i] for i in np.argsort(SR.value_ranks(np.array(vals, dtype=object if t == "STRING" else None), t),
                                        kind="stable").tolist()]
    n = min(int(query.limit), len(vals))
    entries = order_entries(query)
    recs = vals[:n] if (not entries or entries[0][1]) else vals[len(vals) - n:][::-1]
    return [[v] for v in recs], (n, 0, n, seg.num_docs)


def distinct_operator(query, seg, types):
    recs = matching_records(query, seg)
    entries = order_entries(query)
    if entries:
        kept, processed = distinct_order_by(recs, types, entries, int(query.limit))
    else:
        kept, processed = distinct_only(recs, types, int(query.limit))
    return kept, processed


def segment_result(query, seg, types):
    """(records, (numDocsScanned, numEntriesScannedPostFilter, totalDocs), early) of one segment; `early`: the executor
    stopped before the last matching doc."""
    if not seg.num_docs:
        return [], (0, 0, 0), False
    if uses_dictionary_operator(query, seg):
        recs, st = dictionary_operator(query, seg)
        return recs, (st[0], st[2], st[3]), False
    recs, processed = distinct_operator(query, seg, types)
    total = int(np.count_nonzero(SR.filter_mask(query.filter, seg)))
    return recs, (processed, processed * len(query.select_columns), seg.num_docs), processed < total or (
        not order_entries(query) and len(recs) >= int(query.limit) and total > 0)


# ------------------------------------------------------------------ combine / reduce
def merge_tables(tables, types, entries, limit):
    """DistinctTable.mergeTable over `tables` in the given order."""
    if not entries:
        out, seen = [], set()
        for t in tables:
            for r in t:
                if len(out) >= limit:
                    return out
                k = tuple(_ident(v, ty) for v, ty in zip(r, types))
                if k not in seen:
                    seen.add(k)
                    out.append(list(r))
        return out
    recs = unique_records([r for t in tables for r in t], types)
    return distinct_order_by(recs, types, entries, limit)[0]


def reference_server(query, segments):
    """The reference's server result for this segment order: (records, statistics dict)."""
    types = column_types(query, segments)
    entries = order_entries(query)
    tables, docs, post, total = [], 0, 0, 0
    for s in segments:
        recs, st, _ = segment_result(query, s, types)
        tables.append(recs)
        docs += st[0]
        post += st[1]
        total += s.num_docs
    merged = merge_tables(tables, types, entries, int(query.limit))
    if entries:
        merged = sort_records(merged, types, entries)
    return merged, {"numDocsScanned": docs, "numEntriesScannedPostFilter": post, "numTotalDocs": total}


def reference_broker(query, server_tables, types):
    """DistinctDataTableReducer: the servers' tables merged, the limit alone applied, sorted when ORDER BY is present."""
    entries = order_entries(query)
    merged = merge_tables(server_tables, types, entries, int(query.limit))
    return sort_records(merged, types, entries) if entries else merged


# ------------------------------------------------------------------ the deterministic completion
class RefResult:
    def __init__(self):
        self.columns, self.types, self.rows, self.present = [], [], [], 0
        self.matched, self.total_docs, self.stats_defined = 0, 0, True
        self.fast_path = False


def completed_server(query, segments, force_scan=False):
    """What engine.DistinctExecutor is specified to return: the distinct matching records under the completed order, cut
    at the limit; `present` = distinct records before the cut; the statistics where they are defined."""
    res = RefResult()
    bound = [s for s in segments if s.num_docs]
    res.columns = list(query.select_columns)
    res.total_docs = sum(s.num_docs for s in segments)
    if not bound:
        return res
    res.types = column_types(query, segments)
    res.fast_path = not force_scan and all(uses_dictionary_operator(query, s) for s in bound)
    recs = unique_records([r for s in bound for r in matching_records(query, s)], res.types)
    res.present = len(recs)
    res.rows = sort_records(recs, res.types, completed_entries(query))[:int(query.limit)]
    if res.fast_path:
        n = sum(min(int(query.limit), s.column(query.select_columns[0]).cardinality) for s in bound)
        res.matched, res.post = n, n
        return res
    res.matched = sum(int(np.count_nonzero(SR.filter_mask(query.filter, s))) for s in bound)
    res.post = res.matched * len(res.columns)
    res.stats_defined = bool(query.order_by) or res.present < int(query.limit)
    return res


def completed_broker(query, server_rows, types):
    recs = unique_records([r for rows in server_rows for r in rows], types)
    return sort_records(recs, types, completed_entries(query))[:int(query.limit)]
