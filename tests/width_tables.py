"""Tables whose forward indexes have a chosen bit width, and their results in numpy.

The forward-index width nb (1..31) selects the unpacker code that runs (word-straddle shifts, words per lane, DMA chunk
counts, LDS region offsets, the template case taken). pa_segment_add_sv_dict_column takes the width independently of the
cardinality, so a column may be packed at any nb >= bit_length(cardinality - 1); Column.num_bits is what GpuSegment and
the oracle hand on. Two id regimes:

  full    cardinality 2^nb with a real dictionary of 2^nb entries: every bit of every id can be set;
  padded  nb bits over the column's small natural cardinality: the top bits of every id are zero, everything that
          depends on the width alone (bit offset doc * nb mod 32, straddles, chunk counts, offsets, switch case) still runs.

Below the natural width of a column both coincide (cardinality 2^nb).

A table has the columns
  f  INT   filter column            natural 11 bits, 2000 values
  g  INT   group key                natural  5 bits,   24 values
  h  INT   second group key         natural  3 bits,    5 values
  v  LONG / INT / DOUBLE  aggregated value, natural 13 bits, 8000 values
  k  INT   third group key          natural  9 bits,  300 values
  m  INT   multi-value column       natural  7 bits,  100 values, 1..4 values per doc (its rows straddle the
           2048-value boundaries of the value stream); only in the tables whose role it is
  ri INT, rl LONG  raw (no-dictionary) columns of a few values, for the hashed key space
one of which (the role) is packed nb bits wide; the others keep their natural widths (coprime to 32 and different, so no
neighbour's LDS region is aligned by accident). Two segments of 5 * 2048 + 77 and 2048 + 1 docs (several whole wave
tiles and a ragged tail each) hold their own dictionaries (group-key remaps and per-segment value tables are live) or, on
request, share them.

The ids 0, cardinality - 1, 0b0101.. and 0b1010.. (all four carry ones at the top bit and every straddle position in
the full regime) are planted where the addressing changes: docs 0, 31, 32, 63, 64, 1023, 1024, 2047, 2048, the last doc,
the first and last doc of every 8-, 16- and 32-doc lane of the first tile, of every 32-doc lane of the last whole tile,
and the ragged tail's first doc. Every other doc holds a seeded random id. The filter column's id is 0 at the planted
docs (unless f is the role), so `f` ranges starting at the dictionary's first value keep them.

Results are computed from the generated ids and dictionaries (never from the packed bytes, never by the library):
values are integers (DOUBLE columns hold integer-valued doubles) and every sum stays below 2^53, so SUM is exact in
any order and every comparison is bit-exact.
"""
import functools
from dataclasses import dataclass, field
from typing import Dict, List

import numpy as np

from pinot_amd.segment import Column, Segment, pack_bits, write_mv_forward_index

TILE = 2048
SEG_DOCS = (5 * TILE + 77, TILE + 1)
NATURAL = {"f": (11, 2000), "g": (5, 24), "h": (3, 5), "k": (9, 300), "v": (13, 8000), "m": (7, 100)}  # column: (bits, cardinality)
WIDTHS = tuple(range(1, 32))


def cardinality(role, nb, regime):
    """Cardinality of the role column at nb bits: 2^nb when full (or below the natural width), else the natural one."""
    nat = NATURAL[role][1]
    return (1 << nb) if regime == "full" else min(nat, 1 << nb)


def base_regime(role, nb):
    """The regime of the 1..31 sweep: padded from the natural width up, full (cardinality 2^nb) below it."""
    return "padded" if (1 << nb) > NATURAL[role][1] else "full"


def special_ids(card):
    """0, card - 1, 0b0101.. and 0b1010.. within the id bits of the cardinality."""
    bits = max(1, int(card - 1).bit_length())
    mask = (1 << bits) - 1
    out = [0, card - 1, (0x55555555 & mask) % card, (0x2AAAAAAA & mask) % card]
    return np.array(out, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def planted_docs(n):
    """Docs of an n-doc segment that hold special ids (sorted, unique)."""
    docs = {0, 31, 32, 63, 64, 1023, 1024, 2047, 2048, n - 1}
    first = np.arange(min(n, TILE))
    docs.update(first[(first % 8 == 0) | (first % 8 == 7)].tolist())  # 8-, 16- and 32-doc lanes of tile 0
    whole = n // TILE
    if whole > 1:
        last = (whole - 1) * TILE + 32 * np.arange(64)
        docs.update(last.tolist())
        docs.update((last + 31).tolist())
    if n % TILE:
        docs.add(whole * TILE)
    return np.array(sorted(d for d in docs if 0 <= d < n), dtype=np.int64)


def make_ids(rng, n, card):
    """Seeded random ids with the special ids at the planted docs; docs 0, 31, 32, 63 hold card - 1, 0101, 1010, card - 1."""
    ids = rng.integers(0, card, size=n, dtype=np.int64)
    sp = special_ids(card)
    docs = planted_docs(n)
    ids[docs] = sp[rng.integers(0, 4, size=len(docs))]
    for d, k in ((0, 1), (31, 2), (32, 3), (63, 1), (n - 1, 1)):
        if d < n:
            ids[d] = sp[k]
    return ids


def straddling_rows(lengths):
    """Docs of an MV column whose values lie on both sides of a 2048-value boundary of the value stream."""
    ends = np.cumsum(lengths)
    return np.flatnonzero((ends - lengths) // TILE != (ends - 1) // TILE)


def _dictionary(col, card, which, vtype):
    """Sorted dictionary of `card` values of column `col`; which = 0 / 1: the two segments' own dictionaries."""
    i = np.arange(card, dtype=np.int64)
    if col == "f":
        return (3 * i + which).astype(np.int64)
    if col == "g":
        return 10 * i + 5 * which
    if col == "h":
        return 7 * i + 3 * which
    if col == "m":
        return 4 * i + which
    if col == "k":
        return 2 * i + which
    if vtype == "LONG":   # beyond int32
        return (1 << 33) + 1003 * i if which == 0 else -(1 << 33) + 997 * i
    if vtype == "INT":
        return 7 * i - 1000 if which == 0 else 5 * i + 3
    if vtype == "DOUBLE":  # integer-valued
        return (3 * i - 7).astype(np.float64) if which == 0 else (2 * i + 1).astype(np.float64)
    raise ValueError(vtype)


@dataclass
class Table:
    role: str
    nb: int
    regime: str
    vtype: str
    shared: bool
    segments: List[Segment]
    ids: List[Dict[str, np.ndarray]]                 # per segment: column -> dictIds (MV column: list of arrays)
    widths: Dict[str, int] = field(default_factory=dict)

    def card(self, col):
        return self.segments[0].column(col).cardinality

    def values(self, si, col):
        """The values of single-value column `col` in segment si, from its ids and dictionary."""
        c = self.segments[si].column(col)
        return c.raw_values if not c.has_dictionary else c.dictionary[self.ids[si][col]]

    def mv_values(self, si, col="m"):
        """Per doc the values of multi-value column `col` in segment si."""
        d = self.segments[si].column(col).dictionary
        return [d[r] for r in self.ids[si][col]]

    def filter_bounds(self, fraction):
        """(lo, hi) values of `f BETWEEN lo AND hi` that keep the dictIds [0, k) of f in both segments, k about
        fraction * cardinality (at least one id)."""
        k = max(1, int(round(self.card("f") * fraction)))
        return 0, 3 * k - 1


def build_table(role, nb, regime=None, vtype="LONG", shared=False, seed=0):
    """The two-segment table whose column `role` is nb bits wide (see the module docstring)."""
    regime = regime or base_regime(role, nb)
    cols = ["f", "g", "h", "k", "v"] + (["m"] if role == "m" else [])  # (the MV column only where it is the role)
    segs, all_ids, widths = [], [], {}
    for si, n in enumerate(SEG_DOCS):
        rng = np.random.default_rng([seed, nb, si, sum(map(ord, role + regime + vtype))])
        seg = Segment(name="w_%s%d_%s_%d" % (role, nb, regime, si), num_docs=n)
        ids = {}
        for c in cols:
            bits, card = NATURAL[c]
            if c == role:
                bits, card = nb, cardinality(role, nb, regime)
            if card > (1 << bits):
                raise ValueError("%d values do not fit %d bits" % (card, bits))
            which = 0 if shared else si
            dtype = vtype if c == "v" else "INT"
            if shared and si:
                dictionary = segs[0].column(c).dictionary
            else:
                dictionary = _dictionary(c, card, which, vtype)
            col = Column(name=c, data_type=dtype, cardinality=card, num_bits=bits, dictionary=dictionary)
            if c == "m":
                lengths = rng.integers(1, 5, size=n)
                if not len(straddling_rows(lengths)):
                    # no row of this draw lies across a 2048-value boundary: the row that ends at the first one grows by
                    # a value, so the stream always holds a row on both sides of a boundary
                    lengths[np.searchsorted(np.cumsum(lengths), TILE)] += 1
                assert len(straddling_rows(lengths))
                flat = make_ids(rng, int(lengths.sum()), card)
                rows = np.split(flat, np.cumsum(lengths)[:-1])
                col.single_value = False
                col.total_num_values = int(lengths.sum())
                col.max_num_multi_values = int(lengths.max())
                col.fwd_bytes = write_mv_forward_index([r.astype(np.uint32) for r in rows], bits)
                ids[c] = rows
            else:
                cid = make_ids(rng, n, card)
                if c == "f" and role != "f":
                    cid[planted_docs(n)] = 0
                col.fwd_bytes = pack_bits(cid.astype(np.uint32), bits)
                ids[c] = cid
            seg.columns[c] = col
            widths[c] = bits
        seg.columns["ri"] = Column(name="ri", data_type="INT", has_dictionary=False,
                                   raw_values=(rng.integers(0, 7, size=n) * 1000 - 3000).astype(np.int32))
        seg.columns["rl"] = Column(name="rl", data_type="LONG", has_dictionary=False,
                                   raw_values=(rng.integers(0, 5, size=n) - 2).astype(np.int64) * (1 << 40))
        segs.append(seg)
        all_ids.append(ids)
    return Table(role, nb, regime, vtype, shared, segs, all_ids, widths)


# ------------------------------------------------------------------ the reference, in numpy and Python integers

def _to_python(v, dtype):
    return float(v) if dtype == "DOUBLE" else int(v)


def reference(table, aggs, group_by=(), where=None):
    """Expected result of SELECT group_by, aggs FROM t WHERE f BETWEEN lo AND hi GROUP BY group_by over the table.
    aggs: [(function, column or None)], functions COUNT, SUM, MIN, MAX; where: (lo, hi) on f's values, or None.
    Returns (num_docs_scanned, row) without group_by, else (num_docs_scanned, {key values: row}); COUNT is an int, the
    others floats (the engine's intermediate results), computed with exact integer arithmetic."""
    keys_all, cols_all, n_match = [], {c: [] for _, c in aggs if c}, 0
    for si, seg in enumerate(table.segments):
        mask = np.ones(seg.num_docs, dtype=bool)
        if where is not None:
            fv = table.values(si, "f")
            mask = (fv >= where[0]) & (fv <= where[1])
        n_match += int(mask.sum())
        keys_all.append([table.values(si, g)[mask] for g in group_by])
        for c in cols_all:
            cols_all[c].append(table.values(si, c)[mask])
    # (every value is an integer, DOUBLE columns included: int64 arithmetic is exact, and so is the final float)
    cols = {c: np.concatenate(v).astype(np.int64) for c, v in cols_all.items()}
    if group_by:
        keys = [np.concatenate([k[j] for k in keys_all]) for j in range(len(group_by))]
        # one combined key per doc (mixed radix over the columns' distinct values), then the distinct combinations
        comb, parts = np.zeros(n_match, dtype=np.int64), []
        for k in keys:
            u, i = np.unique(k, return_inverse=True)
            comb = comb * len(u) + i.reshape(-1)
            parts.append(u)
        cu, inv = np.unique(comb, return_inverse=True)
        inv, ng = inv.reshape(-1), len(cu)
        uniq = np.zeros((ng, len(keys)), dtype=np.int64)
        for j in range(len(keys) - 1, -1, -1):
            uniq[:, j] = parts[j][cu % len(parts[j])] if len(parts[j]) else 0
            cu = cu // max(len(parts[j]), 1)
    else:
        inv, ng = np.zeros(n_match, dtype=np.int64), 1
    out = []
    for fn, c in aggs:
        if fn == "COUNT":
            out.append(np.bincount(inv, minlength=ng).tolist())
        elif fn == "SUM":
            acc = np.zeros(ng, dtype=np.int64)
            np.add.at(acc, inv, cols[c])
            out.append([float(x) for x in acc.tolist()])
        elif fn in ("MIN", "MAX"):
            seen = np.bincount(inv, minlength=ng) > 0
            acc = np.full(ng, np.iinfo(np.int64).max if fn == "MIN" else np.iinfo(np.int64).min, dtype=np.int64)
            (np.minimum if fn == "MIN" else np.maximum).at(acc, inv, cols[c])
            empty = float("inf") if fn == "MIN" else float("-inf")
            out.append([float(x) if ok else empty for x, ok in zip(acc.tolist(), seen.tolist())])
        else:
            raise ValueError(fn)
    rows = [list(r) for r in zip(*out)]
    if not group_by:
        return n_match, rows[0]
    return n_match, {tuple(int(x) for x in uniq[k]): rows[k] for k in range(ng)}


def sql(aggs, group_by=(), where=None, limit=1_000_000):
    """The SQL text of reference()'s query."""
    sel = list(group_by) + ["COUNT(*)" if fn == "COUNT" else "%s(%s)" % (fn, c) for fn, c in aggs]
    s = "SELECT %s FROM t" % ", ".join(sel)
    if where is not None:
        s += " WHERE f BETWEEN %d AND %d" % where
    if group_by:
        s += " GROUP BY %s LIMIT %d OPTION(numGroupsLimit=%d)" % (", ".join(group_by), limit, limit)
    return s
