"""Pins the checker itself at every forward-index width, without a GPU: the oracle decodes the packed bytes with its own
scalar restatement, so before it serves as a second reference for the GPU width matrix (test_gpu_bit_widths.py) it must
agree with plain numpy over the generated ids and dictionaries (width_tables.reference), at every nb in 1..31 in the
padded regime and in the full regime (a real dictionary of 2^nb values) up to 20 bits; and pack_bits / unpack_bits must
round-trip ids that use all nb bits at every width. Bit-exact: integer values, sums below 2^53."""
import numpy as np
import pytest

import oracle
import width_tables as W
from pinot_amd import parse_sql
from pinot_amd.segment import pack_bits, unpack_bits

FULL_MAX = 20  # a 2^20-entry dictionary (8 MiB) still builds in well under a second
AGGS = [("COUNT", None), ("SUM", "v")]


def _cases():
    for role in ("g", "v"):
        for nb in W.WIDTHS:
            yield role, nb, W.base_regime(role, nb)
            if W.base_regime(role, nb) == "padded" and nb <= FULL_MAX:
                yield role, nb, "full"


@pytest.mark.parametrize("role,nb,regime", list(_cases()))
def test_oracle_group_by_matches_numpy(role, nb, regime):
    t = W.build_table(role, nb, regime)
    q = parse_sql(W.sql(AGGS, ("g",)))
    got = oracle.run_query(q, t.segments)
    docs, groups = W.reference(t, AGGS, ("g",))
    assert got.num_docs_scanned == docs == sum(W.SEG_DOCS)
    assert got.groups == groups


@pytest.mark.parametrize("nb", W.WIDTHS)
def test_oracle_filtered_dense_and_sparse(nb):
    """The filter column at nb bits, a second key and every aggregation function."""
    t = W.build_table("f", nb, vtype="DOUBLE")
    aggs = [("COUNT", None), ("SUM", "v"), ("MIN", "v"), ("MAX", "v")]
    for frac in (0.9, 0.1):
        where = t.filter_bounds(frac)
        got = oracle.run_query(parse_sql(W.sql(aggs, ("g", "h"), where)), t.segments)
        docs, groups = W.reference(t, aggs, ("g", "h"), where)
        assert got.num_docs_scanned == docs > 0
        assert got.groups == groups
        got = oracle.run_query(parse_sql(W.sql(aggs, (), where)), t.segments)
        assert (got.num_docs_scanned, got.row) == W.reference(t, aggs, (), where)


@pytest.mark.parametrize("nb", W.WIDTHS)
def test_pack_unpack_round_trip(nb):
    """Ids over all nb bits (0, 2^nb - 1, 0101.., 1010.. at the planted docs) survive pack_bits -> unpack_bits, and the
    packed stream holds value i at bits [i * nb, (i + 1) * nb), most significant bit first."""
    card = 1 << nb
    for n in W.SEG_DOCS:
        ids = W.make_ids(np.random.default_rng(nb), n, card)
        assert {0, card - 1} <= set(ids.tolist())
        buf = pack_bits(ids.astype(np.uint32), nb)
        assert len(buf) == (n * nb + 7) // 8
        assert np.array_equal(unpack_bits(buf, n, nb).astype(np.int64) & (card - 1), ids)
        for d in (0, 31, 32, 2047, 2048, n - 1):
            word = int.from_bytes(buf[d * nb // 8:d * nb // 8 + 8].tobytes().ljust(8, b"\0"), "big")
            assert (word >> (64 - d * nb % 8 - nb)) & (card - 1) == ids[d]


def test_planted_docs_and_special_ids():
    docs = set(W.planted_docs(W.SEG_DOCS[0]).tolist())
    assert {0, 31, 32, 63, 64, 1023, 1024, 2047, 2048, W.SEG_DOCS[0] - 1, 5 * W.TILE} <= docs
    assert all(32 * l in docs and 32 * l + 31 in docs for l in range(64))
    assert all(16 * l in docs and 16 * l + 15 in docs for l in range(128))
    assert all(4 * W.TILE + 32 * l in docs and 4 * W.TILE + 32 * l + 31 in docs for l in range(64))
    assert W.special_ids(1 << 7).tolist() == [0, 127, 0b1010101, 0b0101010]
    t = W.build_table("v", 9, "full")
    for si in range(2):
        assert set(W.special_ids(512).tolist()) <= set(t.ids[si]["v"][W.planted_docs(W.SEG_DOCS[si])].tolist())
        assert t.segments[si].column("v").num_bits == 9 and t.segments[si].column("g").num_bits == 5
    assert t.segments[0].column("g").dictionary is not t.segments[1].column("g").dictionary
    s = W.build_table("v", 9, "full", shared=True)
    assert s.segments[0].column("v").dictionary is s.segments[1].column("v").dictionary


def _mv_cases():
    for nb in W.WIDTHS:
        yield nb, W.base_regime("m", nb)
        if W.base_regime("m", nb) == "padded" and nb <= 16:
            yield nb, "full"


@pytest.mark.parametrize("nb,regime", list(_mv_cases()))
def test_oracle_mv_stream_matches_numpy(nb, regime):
    """The MV value stream at nb bits: COUNTMV / SUMMV / MINMV / MAXMV behind a filter on f, an ANY leaf (IN) and an
    ALL leaf (NOT IN) on m, and m as the group key (a doc counts once per value), against numpy over the generated rows."""
    t = W.build_table("m", nb, regime)
    where = t.filter_bounds(0.9)
    card = t.card("m")
    want = sorted({int(seg.column("m").dictionary[i]) for seg in t.segments for i in W.special_ids(card).tolist()})
    docs = cnt = total = n_any = n_all = 0
    lo, hi = float("inf"), float("-inf")
    groups = {}
    for si in range(2):
        fv, vv, rows = t.values(si, "f"), t.values(si, "v"), t.mv_values(si)
        for d in np.flatnonzero((fv >= where[0]) & (fv <= where[1])).tolist():
            r = rows[d].tolist()
            docs, cnt, total = docs + 1, cnt + len(r), total + sum(r)
            lo, hi = min(lo, min(r)), max(hi, max(r))
            for x in r:
                g = groups.setdefault((x,), [0, 0])
                g[0] += 1
                g[1] += int(vv[d])
        hit = np.array([bool(set(want) & set(r.tolist())) for r in rows])
        n_any += int(hit.sum())
        n_all += int((~hit).sum())
    sql = "SELECT COUNTMV(m), SUMMV(m), MINMV(m), MAXMV(m) FROM t WHERE f BETWEEN %d AND %d" % where
    got = oracle.run_query(parse_sql(sql), t.segments)
    assert (got.num_docs_scanned, got.row) == (docs, [cnt, float(total), float(lo), float(hi)])
    got = oracle.run_query(parse_sql("SELECT m, COUNT(*), SUM(v) FROM t WHERE f BETWEEN %d AND %d GROUP BY m LIMIT 100000 "
                                     "OPTION(numGroupsLimit=1000000)" % where), t.segments)
    assert got.groups == {k: [c, float(s)] for k, (c, s) in groups.items()}
    lits = ", ".join(map(str, want))
    assert oracle.run_query(parse_sql("SELECT COUNT(*) FROM t WHERE m IN (%s)" % lits), t.segments).row == [n_any]
    assert oracle.run_query(parse_sql("SELECT COUNT(*) FROM t WHERE m NOT IN (%s)" % lits), t.segments).row == [n_all]


def test_mv_rows_straddle_the_value_stream_boundaries():
    """Both segments of an MV table hold rows whose values lie on both sides of a 2048-value boundary."""
    t = W.build_table("m", 7)
    for si in range(2):
        lengths = np.array([len(r) for r in t.ids[si]["m"]])
        rows = W.straddling_rows(lengths)
        assert len(rows) >= 1 and lengths[rows].min() >= 2
        assert t.segments[si].column("m").total_num_values == lengths.sum() > 2 * W.TILE
