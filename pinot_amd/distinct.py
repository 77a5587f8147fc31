"""Distinct queries (SELECT DISTINCT c1, c2, ... [WHERE ...] [ORDER BY ...] [LIMIT n]): the completed order, what one
server returns and the dictionary fast path. Host-side mirror of

  DistinctPlanNode.java:50-78                    one dictionary column without a filter is answered from the dictionary
  DictionaryBasedDistinctOperator.java:56-133    n = min(limit, dictLength) smallest (largest for DESC) values,
                                                 statistics per segment (n, 0, n, numDocs)
  DistinctOperator.java:55-84                    numDocsScanned, numEntriesScannedPostFilter = numDocsScanned x columns
  DistinctTable.java:213-280, DistinctDataTableReducer.java:56,122   the merge and the broker's cut at the limit alone

No GPU code here: engine.DistinctExecutor runs the query, reduce.merge_distinct merges servers.

The completed order. The reference leaves two things open: without ORDER BY the segment tables merge in completion
order, and with ORDER BY on a subset of the columns the tie class at the cut is whatever the heap kept. Here both are
fixed: the ORDER BY entries come first, then every DISTINCT column they do not name, ascending, in select order
(completed_order). Values compare as selection.py's orders (STRING: UTF-16 code units).
"""
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import selection as S


def completed_order(query):
    """[(column index in the DISTINCT list, ascending)], most significant first: the ORDER BY entries, then the columns
    they do not name, ascending, in select order."""
    cols = list(query.select_columns)
    out, named = [], set()
    for o in query.order_by:
        j = cols.index(o.expr)
        if j not in named:
            out.append((j, bool(o.asc)))
            named.add(j)
    out.extend((j, True) for j in range(len(cols)) if j not in named)
    return out


def sort_records(records, column_types, order):
    """Value records (lists in DISTINCT-list order) sorted by the completed order `order`."""
    rows = [list(r) for r in records]
    for j, asc in reversed(order):
        rows.sort(key=lambda r, j=j, dt=column_types[j]: S.row_sort_key(r[j], dt), reverse=not asc)
    return rows


@dataclass
class DistinctResult:
    """What one server returns for a distinct query (DistinctResultsBlock): at most `limit` distinct records, sorted by
    the completed order."""
    columns: List[str]
    column_types: List[str]
    rows: List[list] = field(default_factory=list)   # value records in `columns` order
    present: int = 0                                 # distinct records before the limit
    num_total_docs: int = 0
    # the scan statistics; None = not modelled (no ORDER BY and the limit reached: the reference stops early, at block
    # granularity)
    num_docs_scanned: Optional[int] = None
    num_entries_scanned_in_filter: Optional[int] = None
    num_entries_scanned_post_filter: Optional[int] = None


def dictionary_fast_path(query, segments):
    """DistinctPlanNode.java:50-78: one column, no filter, a dictionary in every segment."""
    return (len(query.select_columns) == 1 and query.filter is None and
            all(s.column(query.select_columns[0]).has_dictionary for s in segments if s.num_docs > 0))


def dictionary_distinct(query, segments):
    """DictionaryBasedDistinctOperator on every segment + the merge: the first (ASC / no ORDER BY) or last (DESC)
    min(limit, dictLength) values of each segment dictionary, merged under the completed order and cut at the limit:
    the union of the segments' own dictionaries in the column's order (a table-wide dictionary shared with other
    servers may hold values no segment here has; they are not this server's). Statistics per segment
    (n_s, 0, n_s, numDocs_s)."""
    name = query.select_columns[0]
    dt = next((s.column(name).data_type for s in segments if s.num_docs > 0), "INT")
    asc = completed_order(query)[0][1]
    res = DistinctResult([name], [dt])
    n_sum = 0
    for s in segments:
        res.num_total_docs += s.num_docs
        if s.num_docs:
            n_sum += min(int(query.limit), s.column(name).cardinality)
    bound = [s.column(name).dictionary for s in segments if s.num_docs]
    vals = list(np.asarray(S.table_order_dictionary(bound, dt)[0]).tolist()) if bound else []
    res.present = len(vals)
    if not asc:
        vals = vals[::-1]
    res.rows = [[v] for v in vals[:int(query.limit)]]
    res.num_docs_scanned = n_sum
    res.num_entries_scanned_in_filter = 0
    res.num_entries_scanned_post_filter = n_sum
    return res
