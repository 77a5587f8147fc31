"""The hashed group-key tables (csrc/pa_keys.h) with keys chosen to collide: probe chains that wrap the table end, tables
exactly full and one past full, many distinct keys of one home slot claimed in one wave step, two-word keys with equal
60-bit fingerprints, and the cross-GPU row merge (pa_merge.hip) with one owner, the reserved slot and an overflowing
table. tests/hash_keys.py builds the keys backwards through mix64 and holds the exact numpy reference.

Every case pins the table at its minimum of 1024 slots (tuning hash_slots_cap), asserts the plan (hashed, key words,
1025 slots with the reserved one) before anything else, lays its keys over two segments of 77 and 2049 docs unless it
fixes the doc count, and compares exactly. The block is moved into a torch buffer (parallel.HashedAccumulators), so the
table itself (the keys section, the counts, the overflow counter PA_ACC_DOCS_U64[1]) is read next to the fetch.

  a  wrapping chain, one word     40 keys of home 1020 in the lanes of one 64-doc step: slots 1020..1023, 0..35
  b  full table                   1024 keys (one home / spread / + INT64_MAX) in 1024 slots: no overflow, exact
  c  one past full                + 3 keys of 4 docs: exactly 12 docs overflow, fetch refuses; the planner's table runs
  d  two words                    fingerprint collisions (in one step and across the segment edge) next to a wrapping
                                  chain; the words 0, -1, INT64_MIN, INT64_MAX in both places; full and one past full
  e  merge by simulated ranks     one owner (a 60-key wrapping chain, every other rank merges nothing), the reserved
                                  slot's group counted once, 1026 keys into 1024 slots: groups 1024, 4 rows over
  f  numGroupsLimit               first-seen trimming over the colliding keys, against the oracle
  g  device-side fetch            a full table through the compaction kernels (block above kFetchWholeBlockBytes)
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

import hash_keys as H
import oracle
from pinot_amd import _lib as L
from pinot_amd import parse_sql
from pinot_amd.engine import GpuQueryExecutor, GpuSegment
from pinot_amd.parallel import SECTION_DTYPE, HashedAccumulators
from test_gpu_parity import SORTED, assert_same

pytestmark = pytest.mark.gpu

# Cases of the list above that the planner makes unreachable: {case: the planner line that does}. None is.
EXCLUDED = {}

SLOTS = 1024
MASK = SLOTS - 1
CAP = {"hash_slots_cap": SLOTS}
MAX = H.INT64_MAX
AGGS = "COUNT(*), SUM(m), MIN(m), MAX(m)"
AGGS_HLL = AGGS + ", DISTINCTCOUNTHLL(m)"
TOTAL = sum(H.SEG_DOCS)
# tile sizes x step- / lane-major tiles, as test_hashed_table_overflow and test_raw_group_by_hashed run them
SCAN = [s | lm for s in (L.PA_QF_STEPS32, L.PA_QF_STEPS16) for lm in (0, L.PA_QF_NO_LANE_MAJOR)]
SCAN_IDS = ["%s-%s" % (s, lm) for s in ("steps32", "steps16") for lm in ("lane_major", "step_major")]
STEPS = [L.PA_QF_STEPS32, L.PA_QF_STEPS16]
E, C = 3, 4  # one past full: E extra keys, every key in C docs


# ------------------------------------------------------------------ key sets (built once)
@functools.lru_cache(maxsize=None)
def one_word(name):
    """chain: one home slot (1023, so the chain wraps at once); spread: homes as a fixed seed draws them; +max: with
    the key INT64_MAX; +e: with E more keys of the same kind."""
    kind, _, extra = name.partition("+")
    n = SLOTS + (E if "e" in extra.split("+") else 0)
    keys = H.chain1(MASK, n, MASK) if kind == "chain" else H.spread1(n, 21)
    if "max" in extra.split("+"):
        keys = np.concatenate([keys, np.array([MAX], dtype=np.int64)])
    return keys


@functools.lru_cache(maxsize=None)
def two_word(name):
    kind, _, extra = name.partition("+")
    n = SLOTS + (E if extra == "e" else 0)
    return H.chain2(MASK, n, MASK) if kind == "chain" else H.spread2(n, 22)


@functools.lru_cache(maxsize=None)
def chain_a():
    return H.chain1(1020, 40, MASK)


FAMILY_HOME, FAMILY = 1010, 7


@functools.lru_cache(maxsize=None)
def colliding_pairs():
    """(keys [24, 2]): a base pair of home 1010 and 6 pairs with its fingerprint and home, a 12-pair chain of home 1022
    (it wraps: slots 1022, 1023, 0..9), a 5-pair chain of home 300."""
    base = H.chain2(FAMILY_HOME, 1, MASK)
    family = np.concatenate([base, H.fp_collisions(int(base[0, 0]), int(base[0, 1]), FAMILY - 1, MASK)])
    return np.concatenate([family, H.chain2(1022, 12, MASK), H.chain2(300, 5, MASK)])


def unequal(n, total, seed):
    """n unequal positive multiplicities that sum to total."""
    p = np.arange(1, n + 1, dtype=np.float64)
    return 1 + np.random.default_rng(seed).multinomial(total - n, p / p.sum())


# ------------------------------------------------------------------ running
class Scanned:
    pass


@contextlib.contextmanager
def scanned(keys, doc_keys, flags=0, aggs=AGGS, tuning=CAP, tail="LIMIT 1000000", seg_docs=None, seed=0, execute=True):
    """The query over the keys laid out in doc order, planned, its plan asserted, its block moved into a torch buffer,
    and scanned. Yields .ex, .views {section kind: tensor}, .rows / .m (key rows and measure per doc), .segs."""
    s = Scanned()
    s.words = 2 if np.asarray(keys).ndim == 2 else 1
    s.segs, s.rows, s.m = H.build_segments(keys, doc_keys, seg_docs=seg_docs, seed=seed)
    s.query = parse_sql(H.sql(s.words, aggs, tail))
    gsegs = [GpuSegment(sg) for sg in s.segs]
    try:
        s.ex = GpuQueryExecutor(s.query, gsegs, flags=flags, tuning=tuning)
        try:
            assert s.ex.hashed and s.ex.key_words == s.words
            if tuning is CAP:
                assert s.ex.num_keys == SLOTS + 1
            s.acc = HashedAccumulators(s.ex, torch.device("cuda", 0))
            s.views = dict(s.acc.views)
            if execute:
                s.ex.execute()
                torch.cuda.synchronize()
            yield s
        finally:
            s.ex.close()
    finally:
        for g in gsegs:
            g.close()


def table(s):
    """(keys int64[1025] or [1025, 3], counts int64[1025], overflow counter) of the scanned block."""
    torch.cuda.synchronize()
    k = s.views[L.PA_ACC_KEYS_I64].cpu().numpy()
    c = s.views[L.PA_ACC_COUNT_U64].cpu().numpy()
    d = s.views[L.PA_ACC_DOCS_U64].cpu().numpy()
    return (k if s.words == 1 else k.reshape(-1, 3)), c, int(d[1])


def groups_of(res, hll=False):
    """An IntermediateResult's groups as {key tuple of ints: [count, sum, min, max]} (and {key: HLL registers})."""
    out, regs = {}, {}
    for k, v in res.groups.items():
        key = tuple(int(x) for x in k)
        out[key] = [int(v[0]), float(v[1]), float(v[2]), float(v[3])]
        assert isinstance(v[0], (int, np.integer))
        if hll:
            regs[key] = v[4].registers
    assert len(out) == len(res.groups)
    return (out, regs) if hll else out


def assert_exact(s, res=None, rows=None, m=None, log2m=None):
    """The fetch equals the numpy reference over the docs: the same keys, every value equal."""
    res = s.ex.fetch() if res is None else res
    rows, m = (s.rows, s.m) if rows is None else (rows, m)
    want = H.reference(rows, m)
    if log2m is None:
        got = groups_of(res)
    else:
        got, regs = groups_of(res, hll=True)
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:4]
    bad = [(k, got[k], want[k]) for k in want if got[k] != want[k]]
    assert not bad, bad[:4]
    if log2m is not None:
        want_regs = H.reference_hll(rows, m, log2m)
        assert all(np.array_equal(regs[k], want_regs[k]) for k in want)
    return res


def chain_slots(home, n):
    return {(home + i) & MASK for i in range(n)}


# ------------------------------------------------------------------ a. wrapping chain, one word
@pytest.mark.parametrize("flags", SCAN, ids=SCAN_IDS)
def test_wrapping_chain_claimed_in_one_step(flags):
    """40 distinct keys of home slot 1020 sit in docs 0..39: 40 lanes of one 64-doc step probe one chain at once (a CAS
    that loses to another key moves on), later docs repeat them. The table holds each key once in the slots 1020..1023,
    0..35: the chain wrapped, the reserved slot 1024 was not probed, and the helper's mix64 is the device's."""
    keys = chain_a()
    docs = H.layout(unequal(40, TOTAL, 1), pinned=[(i, i) for i in range(40)], seed=1)
    with scanned(keys, docs, flags) as s:
        k, c, over = table(s)
        assert set(np.flatnonzero(k[:SLOTS] != MAX).tolist()) == chain_slots(1020, 40)
        assert sorted(k[:SLOTS][k[:SLOTS] != MAX].tolist()) == sorted(keys.tolist())
        assert k[SLOTS] == MAX and c[SLOTS] == 0 and over == 0
        res = assert_exact(s)
        assert res.num_docs_scanned == TOTAL and len(res.groups) == 40


# ------------------------------------------------------------------ b. full table, c. one past full (one word)
@pytest.mark.parametrize("flags", SCAN, ids=SCAN_IDS)
@pytest.mark.parametrize("keyset", ["chain", "spread", "chain+max", "spread+max"])
def test_full_table_one_word(keyset, flags):
    """1024 distinct keys in 1024 slots (the probe bound `probe <= mask` reaches the last free slot), every key in 4 docs:
    no overflow, every slot taken, every group exact. With INT64_MAX (its own reserved slot) 1025 groups."""
    keys = one_word(keyset)
    docs = H.layout(np.full(len(keys), C), seed=2)
    with scanned(keys, docs, flags) as s:
        k, c, over = table(s)
        assert over == 0
        assert (k[:SLOTS] != MAX).all() and (c[:SLOTS] == C).all() and c[SLOTS] == (C if "max" in keyset else 0)
        res = assert_exact(s)
        assert len(res.groups) == len(keys) == SLOTS + ("max" in keyset)
        assert res.num_docs_scanned == C * len(keys)


@pytest.mark.parametrize("flags", SCAN, ids=SCAN_IDS)
@pytest.mark.parametrize("keyset", ["chain+e", "spread+e", "chain+e+max", "spread+e+max"])
def test_one_past_full_one_word(keyset, flags):
    """3 keys more than slots, every key in 4 docs: whichever keys lose the race, every doc of a loser is dropped and
    counted, so the overflow counter is exactly 3 * 4, the 1024 winners hold 4 docs each, INT64_MAX's docs are never
    counted, and fetch refuses. The planner's own table (twice the docs) holds them all."""
    keys = one_word(keyset)
    docs = H.layout(np.full(len(keys), C), seed=3)
    with scanned(keys, docs, flags) as s:
        k, c, over = table(s)
        assert over == E * C
        assert (k[:SLOTS] != MAX).all() and len(set(k[:SLOTS].tolist())) == SLOTS and set(k[:SLOTS].tolist()) <= set(keys.tolist())
        assert (c[:SLOTS] == C).all() and c[SLOTS] == (C if "max" in keyset else 0)
        with pytest.raises(L.PinotAmdError, match="group-key table overflow"):
            s.ex.fetch()
    with scanned(keys, docs, flags, tuning=None) as s:
        assert s.ex.num_keys > 2 * len(keys)
        assert table(s)[2] == 0
        assert len(assert_exact(s).groups) == len(keys)


# ------------------------------------------------------------------ d. two-word keys
@pytest.mark.parametrize("flags", SCAN, ids=SCAN_IDS)
def test_fingerprint_collisions(flags):
    """7 pairs with one fingerprint and one home slot (1010): a lane whose fingerprint matches a slot compares k0 / k1
    and moves on to the next slot. Their first docs are 7 lanes of one 64-doc step (docs 0..6, with a 12-pair chain of
    home 1022 in docs 7..18), and they meet again in docs 74..80, across the segment edge (other workgroups). The 7 pairs
    lie in the slots 1010..1016, state words equal in the fingerprint bits, READY and not BUSY; the chain wrapped."""
    keys = colliding_pairs()
    pinned = [(i, i) for i in range(FAMILY + 12)] + [(74 + i, i) for i in range(FAMILY)]
    docs = H.layout(unequal(len(keys), TOTAL, 4), pinned=pinned, seed=4)
    with scanned(keys, docs, flags) as s:
        k, c, over = table(s)
        occ = np.flatnonzero(k[:SLOTS, 2] != MAX)
        fam = [(FAMILY_HOME + i) & MASK for i in range(FAMILY)]
        assert set(occ.tolist()) == set(fam) | chain_slots(1022, 12) | chain_slots(300, 5)
        assert sorted(map(tuple, k[occ, :2].tolist())) == sorted(map(tuple, keys.tolist()))  # each pair once
        assert sorted(map(tuple, k[fam, :2].tolist())) == sorted(map(tuple, keys[:FAMILY].tolist()))
        fp = H.fp2(int(keys[0, 0]), int(keys[0, 1]))
        assert (k[fam, 2] & H.FP_MASK == fp).all()
        assert (k[occ, 2] & H.KEY_READY != 0).all() and (k[occ, 2] & H.KEY_BUSY == 0).all()
        assert (k[SLOTS] == MAX).all() and over == 0
        res = assert_exact(s)
        assert res.num_docs_scanned == TOTAL and len(res.groups) == len(keys)


@pytest.mark.parametrize("flags", SCAN, ids=SCAN_IDS)
def test_two_word_edge_values(flags):
    """Every (a, b) over 0, -1, INT64_MIN, INT64_MAX, so each pair runs with its mirror (b, a), (INT64_MAX, INT64_MAX)
    among them (the empty marker is a state word: no key word is special), next to the colliding pairs."""
    v = [0, -1, H.INT64_MIN, MAX]
    keys = np.concatenate([np.array([(a, b) for a in v for b in v], dtype=np.int64), colliding_pairs()])
    docs = H.layout(unequal(len(keys), TOTAL, 5), pinned=[(i, i) for i in range(len(keys))], seed=5)
    with scanned(keys, docs, flags) as s:
        assert table(s)[2] == 0
        res = assert_exact(s)
        assert len(res.groups) == len(keys) and (MAX, MAX) in groups_of(res)


@pytest.mark.parametrize("flags", SCAN, ids=SCAN_IDS)
@pytest.mark.parametrize("keyset", ["chain", "spread"])
def test_full_table_two_words(keyset, flags):
    keys = two_word(keyset)
    docs = H.layout(np.full(len(keys), C), seed=6)
    with scanned(keys, docs, flags) as s:
        k, c, over = table(s)
        assert over == 0 and (k[:SLOTS, 2] != MAX).all() and (c[:SLOTS] == C).all() and c[SLOTS] == 0
        assert len(assert_exact(s).groups) == SLOTS


@pytest.mark.parametrize("flags", SCAN, ids=SCAN_IDS)
@pytest.mark.parametrize("keyset", ["chain+e", "spread+e"])
def test_one_past_full_two_words(keyset, flags):
    keys = two_word(keyset)
    docs = H.layout(np.full(len(keys), C), seed=7)
    with scanned(keys, docs, flags) as s:
        k, c, over = table(s)
        assert over == E * C
        assert (k[:SLOTS, 2] != MAX).all() and (c[:SLOTS] == C).all()
        held = set(map(tuple, k[:SLOTS, :2].tolist()))
        assert len(held) == SLOTS and held <= set(map(tuple, keys.tolist()))
        with pytest.raises(L.PinotAmdError, match="group-key table overflow"):
            s.ex.fetch()
    with scanned(keys, docs, flags, tuning=None) as s:
        assert s.ex.num_keys > 2 * len(keys)
        assert table(s)[2] == 0
        assert len(assert_exact(s).groups) == len(keys)


# ------------------------------------------------------------------ e. merge by simulated ranks
@contextlib.contextmanager
def ranks(keys, held, docs_of, seg_docs=None):
    """One scanned executor per rank (held[w]: the indexes into keys that rank w holds, docs_of(w, n held) -> doc order
    over them), the rows exchanged by hand as test_library_pack_and_merge_rows_across_simulated_ranks does. Yields
    (scanned ranks, packed = [(rows tensor grouped by owner, rows per owner)])."""
    with contextlib.ExitStack() as stack:
        rs = [stack.enter_context(scanned(keys[h], docs_of(w, len(h)), aggs=AGGS_HLL, seed=100 + w, seg_docs=seg_docs))
              for w, h in enumerate(held)]
        for s in rs:
            assert table(s)[2] == 0  # (no rank's own scan overflows)
        yield rs, [s.acc.rows.pack(len(held)) for s in rs]


def rows_for(packed, w):
    parts = []
    for buf, counts in packed:
        lo = sum(counts[:w])
        parts.append(buf[lo:lo + counts[w]])
    return torch.cat(parts)


def owned_chain(words, world, n):
    """n keys of home slot 1000 that rank 0 owns; two words: the last 3 share the first one's fingerprint."""
    t = H.Tally()
    if words == 1:
        return H.take(n, H.owned_by(0, world, H.iter_chain1(1000, MASK, tally=t)), MASK, t)
    chain = H.take(n - 3, H.owned_by(0, world, H.iter_chain2(1000, MASK, tally=t)), MASK, t)
    t = H.Tally()
    coll = H.take(3, H.owned_by(0, world, H.iter_fp_collisions(int(chain[0, 0]), int(chain[0, 1]), MASK, tally=t)), MASK, t)
    return np.concatenate([chain, coll])


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("words", [1, 2])
def test_merge_one_owner(words, world):
    """Every rank holds the same 60 keys, one wrapping chain (home 1000) that rank 0 owns whole: every rank's rows for
    one key go into one chain at once (HLL registers combined by byte max on contended slots), the other ranks receive
    nothing, merge zero rows and fetch zero groups with their numDocsScanned kept."""
    keys = owned_chain(words, world, 60)
    own = H.owner1(keys, world) if words == 1 else H.owner2(keys[:, 0], keys[:, 1], world)
    assert (own == 0).all()
    held = [np.arange(60)] * world
    with ranks(keys, held, lambda w, n: H.layout(unequal(n, TOTAL, 30 + w), seed=30 + w)) as (rs, packed):
        for _, counts in packed:
            assert counts == [60] + [0] * (world - 1)
        groups, over = rs[0].acc.rows.merge(rows_for(packed, 0))
        assert (groups, over) == (60, 0)
        for s in rs[1:]:
            assert s.acc.rows.merge(rows_for(packed, rs.index(s))) == (0, 0)
            res = s.ex.fetch()
            assert len(res.groups) == 0 and res.num_docs_scanned == TOTAL
        k, c, _ = table(rs[0])
        state = k if words == 1 else k[:, 2]
        assert set(np.flatnonzero(state[:SLOTS] != MAX).tolist()) == chain_slots(1000, 60)
        res = assert_exact(rs[0], rows=np.concatenate([s.rows for s in rs]), m=np.concatenate([s.m for s in rs]), log2m=8)
        assert res.num_docs_scanned == TOTAL  # (this rank's own: the broker sums the ranks')


@pytest.mark.parametrize("world", [2, 3])
def test_merge_reserved_slot(world):
    """INT64_MAX held by every rank next to 80 other keys: its owner receives `world` rows of it, counts its group once
    (the reserved slot mask + 1 is its own marker) and combines their accumulators exactly."""
    keys = np.concatenate([H.spread1(80, 40), np.array([MAX], dtype=np.int64)])
    own = H.owner1(keys, world)
    held = [np.arange(len(keys))] * world
    with ranks(keys, held, lambda w, n: H.layout(unequal(n, TOTAL, 40 + w), seed=40 + w)) as (rs, packed):
        all_rows, all_m = np.concatenate([s.rows for s in rs]), np.concatenate([s.m for s in rs])
        for w, s in enumerate(rs):
            assert packed[w][1] == [int((own == r).sum()) for r in range(world)]
            groups, over = s.acc.rows.merge(rows_for(packed, w))
            assert (groups, over) == (int((own == w).sum()), 0)
            mine = np.isin(all_rows, keys[own == w])
            res = assert_exact(s, rows=all_rows[mine], m=all_m[mine], log2m=8)
            assert ((MAX,) in groups_of(res)) == (own[-1] == w)
        assert sum(int((own == w).sum()) for w in range(world)) == len(keys)


@pytest.mark.parametrize("words", [1, 2])
def test_merge_overflow(words):
    """1026 keys that rank 0 of 3 owns, each held by two ranks (342 keys each by ranks 0 + 1, 1 + 2, 0 + 2: 684 keys a
    rank, no scan overflows): rank 0 receives 2052 rows for 1024 slots, stores 1024 groups and reports the 2 rows of each
    of the 2 keys that found no slot."""
    n, world = 1026, 3
    t = H.Tally()
    it = H.iter_chain1(7, MASK, tally=t) if words == 1 else H.iter_chain2(7, MASK, tally=t)
    keys = H.take(n, H.owned_by(0, world, it), MASK, t)
    third = np.arange(n).reshape(3, n // 3)
    held = [np.concatenate([third[0], third[2]]), np.concatenate([third[0], third[1]]), np.concatenate([third[1], third[2]])]
    with ranks(keys, held, lambda w, k: H.layout(np.full(k, 2), seed=50 + w)) as (rs, packed):
        for _, counts in packed:
            assert counts == [684, 0, 0]
        groups, over = rs[0].acc.rows.merge(rows_for(packed, 0))
        assert groups == 1024
        assert over == (n - SLOTS) * 2 == 4
        for w in (1, 2):
            assert rs[w].acc.rows.merge(rows_for(packed, w)) == (0, 0)


# ------------------------------------------------------------------ f. numGroupsLimit over colliding keys
@pytest.mark.parametrize("steps", STEPS, ids=["steps32", "steps16"])
@pytest.mark.parametrize("words", [1, 2])
def test_num_groups_limit_over_colliding_keys(words, steps):
    """First-seen trimming (the first-position passes over the hashed table and their own first_slot table) with the
    colliding keys first in docId order: the same groups as the oracle's first-seen maps."""
    if words == 1:
        keys = np.concatenate([chain_a(), H.spread1(300, 60)])
    else:
        keys = np.concatenate([colliding_pairs(), H.spread2(300, 61)])
    lead = 40 if words == 1 else len(colliding_pairs())
    docs = H.layout(unequal(len(keys), TOTAL, 60), pinned=[(i, i) for i in range(lead)], seed=60)
    with scanned(keys, docs, steps, tail="LIMIT 1000000 OPTION(numGroupsLimit=25)", execute=False) as s:
        assert s.ex.stats()["plan"]["limit_trimming"] == int(SORTED)
        got = s.ex.run()
        exp = oracle.run_query(s.query, s.segs)
        assert_same(got, exp)
        assert got.num_groups_limit_reached and 25 <= len(got.groups) <= 50
        want = H.reference(s.rows, s.m)  # (whole groups: a kept key keeps every doc of its segment at least)
        assert set(groups_of(got)) <= set(want)


# ------------------------------------------------------------------ g. device-side fetch of a full table
@pytest.mark.parametrize("steps", STEPS, ids=["steps32", "steps16"])
@pytest.mark.parametrize("keyset", ["chain", "spread+max"])
def test_device_fetch_of_a_full_table(keyset, steps):
    """A full table whose block is above the whole-block copy's size (HLL registers at log2m 11: 2 KiB a slot), so the
    fetch compacts on the device: the compaction kernels read a table without an empty slot."""
    keys = one_word(keyset)
    docs = H.layout(np.full(len(keys), C), seed=8)
    with scanned(keys, docs, steps, aggs=AGGS + ", DISTINCTCOUNTHLL(m, 11)") as s:
        total = sum(n * torch.empty(0, dtype=SECTION_DTYPE[kind]).element_size() for kind, _, n in s.ex.sections())
        assert total > 1 << 20 and int(L.lib().pa_query_accumulator_bytes(s.ex.handle)) > 1 << 20
        k, c, over = table(s)
        assert over == 0 and (k[:SLOTS] != MAX).all()
        assert len(assert_exact(s, log2m=11).groups) == len(keys)
