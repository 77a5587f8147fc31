"""Selection queries (SELECT columns | * ... [ORDER BY ...] [LIMIT [offset,] n]): what the server's result holds and the
orders it is sorted by. Host-side mirror of

  SelectionOperatorUtils.extractExpressions   the result's columns: the ORDER BY columns first (each once), then the
                                              rest of the select list; `*` = every physical column of the schema
  SelectionOrderByOperator.java:108-112       the comparator: column by column, DESC reversed
  SelectionOrderByOperator.java:175,239,300   numEntriesScannedPostFilter

No GPU code here: engine.SelectionExecutor runs the query, reduce.merge_selection merges servers.

Orders. The GPU sorts one unsigned key per doc (include/pinot_amd.h, "selection queries"), so every value order is
restated as an order of unsigned integers or byte strings:
  INT / LONG      the value
  FLOAT / DOUBLE  Double.compare: -0.0 < 0.0, every NaN equal and greatest (float_order_bits)
  STRING          String.compareTo = UTF-16 code units, which is the byte order of the UTF-16-BE encoding. Code-point
                  order (Python's, numpy's) differs for U+E000..U+FFFF against supplementary characters.
"""
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np


def float_order_bits(values):
    """uint64 image of float values whose unsigned order is Double.compare's (FLOAT widened to double first, which keeps
    the order; every NaN becomes the canonical one)."""
    a = np.ascontiguousarray(values, dtype=np.float64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = np.uint64(0x7FF8000000000000)
    neg = (b >> np.uint64(63)).astype(bool)
    return np.where(neg, ~b, b | np.uint64(1 << 63))


def utf16_key(s):
    """A Python str as bytes whose order is Java's String.compareTo."""
    return str(s).encode("utf-16-be", "surrogatepass")


def order_keys(values, data_type):
    """One sortable key per value, in the column's order (module docstring): a list for STRING (bytes), else an array."""
    if data_type == "STRING":
        return [utf16_key(v) for v in np.asarray(values).tolist()]
    if data_type in ("FLOAT", "DOUBLE"):
        return float_order_bits(values)
    return np.asarray(values, dtype=np.int64)


def table_order_dictionary(dictionaries, data_type):
    """The table-wide dictionary of an ORDER BY column: the union of the segments' dictionary values, ascending in the
    column's order, one entry per distinct key. Returns (values, keys)."""
    vals = np.concatenate([np.asarray(d) for d in dictionaries])
    keys = order_keys(vals, data_type)
    if data_type == "STRING":
        first = {}
        for i, k in enumerate(keys):
            first.setdefault(k, i)
        ks = sorted(first)
        return vals[[first[k] for k in ks]], ks
    uk, idx = np.unique(keys, return_index=True)
    return vals[idx], uk


def order_remap(table_keys, dictionary, data_type):
    """int32[len(dictionary)]: the rank of every value of a segment dictionary in the table-wide dictionary."""
    keys = order_keys(dictionary, data_type)
    if data_type == "STRING":
        rank = {k: i for i, k in enumerate(table_keys)}
        try:
            return np.array([rank[k] for k in keys], dtype=np.int32)
        except KeyError:
            raise ValueError("table dictionary misses values of a bound segment")
    tk = np.asarray(table_keys)
    r = np.searchsorted(tk, keys)
    if len(keys) and (r.max(initial=0) >= len(tk) or not np.array_equal(tk[np.minimum(r, len(tk) - 1)], keys)):
        raise ValueError("table dictionary misses values of a bound segment")
    return r.astype(np.int32)


def result_columns(query, schema_columns):
    """SelectionOperatorUtils.extractExpressions: deduplicated ORDER BY columns, then the remaining select columns
    (`*`: the schema's physical columns, by name)."""
    out = []
    for o in query.order_by:
        if o.expr not in out:
            out.append(o.expr)
    select = sorted(schema_columns) if query.select_star else list(query.select_columns)
    for c in select:
        if c not in out:
            out.append(c)
    return out


def select_list(query, schema_columns):
    """The broker's output columns (the select list as written; `*`: the schema's physical columns, by name)."""
    return sorted(schema_columns) if query.select_star else list(query.select_columns)


def post_filter_entries(segment_matched, num_rows, num_order_by_columns, num_other_columns):
    """numEntriesScannedPostFilter of SelectionOrderByOperator over segments that matched segment_matched docs each: every
    ordered column is read for every matching doc (SelectionOrderByOperator.java:175); when other columns are projected,
    they are read only for the rows a segment keeps (:239, :300)."""
    matched = [int(m) for m in segment_matched]
    total = sum(matched) * num_order_by_columns
    if num_other_columns:
        total += sum(min(int(num_rows), m) for m in matched) * num_other_columns
    return total


@dataclass
class SelectionResult:
    """What one server returns for a selection (SelectionResultsBlock): rows under the ORDER BY comparator, ties by
    (segment, doc); without ORDER BY the first matching docs in that order."""
    columns: List[str]
    column_types: List[str]
    rows: List[list] = field(default_factory=list)        # values in `columns` order
    segments: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))  # per row: segment index, doc id and
    docs: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))      # the GPU's sort key
    keys: np.ndarray = field(default_factory=lambda: np.zeros(0, np.uint64))
    num_total_docs: int = 0
    # the scan statistics; None = not modelled (no ORDER BY, or ordered by a sorted column first: the reference stops
    # early there)
    num_docs_scanned: Optional[int] = None
    num_entries_scanned_in_filter: Optional[int] = None
    num_entries_scanned_post_filter: Optional[int] = None


def row_sort_key(value, data_type):
    """One value's key in its column's order (the broker merges decoded rows)."""
    if data_type == "STRING":
        return utf16_key(value)
    if data_type in ("FLOAT", "DOUBLE"):
        return int(float_order_bits([value])[0])
    return int(value)
