"""Group keys with chosen places in the hashed group-key tables (csrc/pa_keys.h), and their results in numpy.

The tables are open addressing with linear probing: a one-word key's home slot is mix64(key) & mask (ht_slot1), a
two-word key's mix64(k0 ^ mix64(k1)) & mask with the 60-bit fingerprint mix64(k1 ^ mix64(k0 + GOLD)) in its state word
(ht_slot2), and the cross-GPU merge gives a key to rank owner_of(key) (pa_merge.hip). GROUP BY over raw LONG columns
hands the column values to these functions unchanged (one column: k0 = a; two: k0 = a, k1 = b), and mix64 is a bijection
of the 64-bit words, so keys are built backwards from the slot, the fingerprint and the owner they are to have:

  chain1        keys unmix64(home + (mask + 1) * j): any number of one-word keys with one home slot
  chain2        pairs (unmix64(home + (mask + 1) * j) ^ mix64(j), j): the same for two words, fingerprints all different
  fp_collisions for a pair's fingerprint F and any other k1', the 16 words k0' = unmix64(unmix64(F + t * 2^60) ^ k1') - GOLD
                (t = 0..15: the 4 bits above the fingerprint) have the fingerprint F; one candidate in mask + 1 also has
                the pair's home slot
  spread1 / 2   seeded random keys (homes as they fall)
  owned_by      a filter over any of the iterators: owner_of does not depend on mix64(key) & mask, so about one
                candidate in `world` passes

Every function here restates the device's arithmetic on Python integers (and on numpy uint64 arrays where given arrays);
tests/test_hash_keys.py holds them against parallel.py's torch restatements, and the GPU tests against the device (the
occupied slots of a scanned table are where home1 / home2 say). Searches count their candidates (Tally) and stop with an
error at 64 x (table size) candidates per key asked for, so a broken construction fails and does not spin.

Results (reference): COUNT(*), SUM(m), MIN(m), MAX(m) per distinct key row by np.unique and int64 arithmetic over an INT
measure, every sum far below 2^53, so the comparison is exact; HLL registers by hll.slot_rank over the measure's values.
"""
import itertools

import numpy as np

M64 = (1 << 64) - 1
INT64_MAX = (1 << 63) - 1
INT64_MIN = -(1 << 63)
C1 = 0xff51afd7ed558ccd
C2 = 0xc4ceb9fe1a85ec53
C1_INV = pow(C1, -1, 1 << 64)
C2_INV = pow(C2, -1, 1 << 64)
GOLD = 0x9E3779B97F4A7C15
FP_BITS = 60
FP_MASK = (1 << FP_BITS) - 1
KEY_READY = 1 << 60
KEY_BUSY = 1 << 61
CANDIDATES_PER_KEY = 64  # x table size: the search bound of every constructor


def _is_array(x):
    return isinstance(x, np.ndarray)


def _u64(x):
    """The 64-bit word of x, unsigned: a Python int, or a uint64 array (a copy)."""
    if _is_array(x):
        return x.astype(np.int64).view(np.uint64).copy() if x.dtype != np.uint64 else x.copy()
    return int(x) & M64


def signed(x):
    """The 64-bit word of x as a signed value: a Python int, or an int64 array."""
    if _is_array(x):
        return x.view(np.int64) if x.dtype == np.uint64 else x.astype(np.int64)
    x = int(x) & M64
    return x - (1 << 64) if x >> 63 else x


def _mul(x, c):
    return x * np.uint64(c) if _is_array(x) else (x * c) & M64


def _xs33(x):
    return x ^ (x >> np.uint64(33)) if _is_array(x) else x ^ (x >> 33)


def mix64(x):
    """pa_keys.h mix64 (unsigned result)."""
    x = _u64(x)
    return _xs33(_mul(_xs33(_mul(_xs33(x), C1)), C2))


def unmix64(y):
    """mix64's inverse: x ^ (x >> 33) undoes itself (33 >= 32), the multipliers are odd and so invertible mod 2^64."""
    y = _u64(y)
    return _xs33(_mul(_xs33(_mul(_xs33(y), C2_INV)), C1_INV))


def home1(key, mask):
    return mix64(key) & (np.uint64(mask) if _is_array(key) else mask)


def home2(k0, k1, mask):
    return mix64(_u64(k0) ^ mix64(k1)) & (np.uint64(mask) if _is_array(k0) else mask)


def fp2(k0, k1):
    g = np.uint64(GOLD) if _is_array(k0) else GOLD
    s = _u64(k0) + g
    if not _is_array(k0):
        s &= M64
    return mix64(_u64(k1) ^ mix64(s)) & (np.uint64(FP_MASK) if _is_array(k0) else FP_MASK)


def owner1(key, world):
    """pa_merge.hip owner_of of a one-word key."""
    if _is_array(key):
        k = signed(key)
        h = k ^ (k >> np.int64(31))
        h = (h.view(np.uint64) * np.uint64(GOLD)).view(np.int64)
        return ((h >> np.int64(33)) & np.int64(0x7FFFFFFF)) % np.int64(world)
    k = signed(key)
    h = signed((k ^ (k >> 31)) * GOLD)
    return ((h >> 33) & 0x7FFFFFFF) % world


def owner2(k0, k1, world):
    return owner1(signed(_u64(k0) ^ mix64(k1)), world)


class Tally:
    """Counts the candidates a search looks at; past `bound` of them (set by take) the search raises."""

    def __init__(self):
        self.tried = 0
        self.bound = None


def _counted(it, tally):
    for x in it:
        if tally is not None:
            tally.tried += 1
            if tally.bound is not None and tally.tried > tally.bound:
                raise RuntimeError("key search: more than %d candidates tried" % tally.bound)
        yield x


def iter_chain1(home, mask, start=1, tally=None):
    """One-word keys with home slot `home`, never INT64_MAX: unmix64(home + (mask + 1) * j), j = start, start + 1, .."""
    assert 0 <= home <= mask
    for j in _counted(itertools.count(start), tally):
        k = signed(unmix64((home + (mask + 1) * j) & M64))
        if k != INT64_MAX:
            yield k


def iter_chain2(home, mask, start=1, tally=None):
    """Pairs with home slot `home` and fingerprints that differ from every earlier pair's."""
    assert 0 <= home <= mask
    seen = set()
    for j in _counted(itertools.count(start), tally):
        k0 = unmix64((home + (mask + 1) * j) & M64) ^ mix64(j)
        f = fp2(k0, j)
        if f not in seen:
            seen.add(f)
            yield signed(k0), j


def iter_fp_collisions(k0, k1, mask, start=1, tally=None):
    """Pairs other than (k0, k1) with its fingerprint and its home slot."""
    F, home = fp2(k0, k1), home2(k0, k1, mask)
    cand = ((b, t) for b in itertools.count(start) for t in range(1 << (64 - FP_BITS)))
    for b, t in _counted(cand, tally):
        a = (unmix64(unmix64(F + (t << FP_BITS)) ^ b) - GOLD) & M64
        if home2(a, b, mask) == home and (signed(a), b) != (signed(k0), signed(k1)):
            yield signed(a), b


def iter_spread1(seed):
    """Seeded random one-word keys, distinct, never INT64_MAX."""
    rng = np.random.default_rng(seed)
    seen = set()
    while True:
        for k in rng.integers(INT64_MIN, INT64_MAX, size=256, dtype=np.int64, endpoint=True).tolist():
            if k != INT64_MAX and k not in seen:
                seen.add(k)
                yield k


def iter_spread2(seed):
    rng = np.random.default_rng(seed)
    seen = set()
    while True:
        for p in rng.integers(INT64_MIN, INT64_MAX, size=(256, 2), dtype=np.int64, endpoint=True).tolist():
            if tuple(p) not in seen:
                seen.add(tuple(p))
                yield tuple(p)


def owned_by(rank, world, keys_iter):
    """The keys of an iterator (one-word keys, or pairs) that rank `rank` of `world` owns in the merge."""
    for k in keys_iter:
        own = owner2(k[0], k[1], world) if isinstance(k, tuple) else owner1(k, world)
        if own == rank:
            yield k


def take(n, keys_iter, mask, tally=None):
    """The first n keys of an iterator as a signed int64 array ([n] or [n, 2]); raises once the search has looked at more
    than 64 x (table size) candidates per key asked for (when the iterator counts into `tally`)."""
    if tally is not None:  # (the candidate stream itself carries the bound: a search that finds nothing still ends)
        tally.bound = tally.tried + CANDIDATES_PER_KEY * (mask + 1) * max(n, 1)
    out = [next(keys_iter) for _ in range(n)]
    words = 2 if out and isinstance(out[0], tuple) else 1
    return np.array(out, dtype=np.int64).reshape((n, 2) if words == 2 else (n,))


def chain1(home, n, mask, start=1, tally=None):
    tally = tally or Tally()
    return take(n, iter_chain1(home, mask, start, tally), mask, tally)


def chain2(home, n, mask, start=1, tally=None):
    tally = tally or Tally()
    return take(n, iter_chain2(home, mask, start, tally), mask, tally)


def fp_collisions(k0, k1, n, mask, start=1, tally=None):
    tally = tally or Tally()
    return take(n, iter_fp_collisions(k0, k1, mask, start, tally), mask, tally)


def spread1(n, seed):
    return take(n, iter_spread1(seed), 0)


def spread2(n, seed):
    return take(n, iter_spread2(seed), 0)


# ------------------------------------------------------------------ tables
SEG_DOCS = (77, 2049)   # first occurrences straddle a segment edge and a 2048-doc tile edge
MEASURE = (-500, 500)   # the INT measure's value range


def layout(mult, pinned=(), seed=0):
    """A doc order: int64[sum(mult)] of key indexes in which key i occurs mult[i] times, doc `pos` holds key `ki` for
    every (pos, ki) of `pinned`, and the other occurrences fill the other docs in seeded random order."""
    mult = np.asarray(mult, dtype=np.int64)
    total = int(mult.sum())
    left = mult.copy()
    docs = np.full(total, -1, dtype=np.int64)
    for pos, ki in pinned:
        assert docs[pos] < 0 and left[ki] > 0, (pos, ki)
        docs[pos] = ki
        left[ki] -= 1
    rest = np.repeat(np.arange(len(mult), dtype=np.int64), left)
    np.random.default_rng(seed).shuffle(rest)
    docs[docs < 0] = rest
    assert np.array_equal(np.bincount(docs, minlength=len(mult)), mult)
    return docs


def build_segments(keys, doc_keys, seg_docs=None, seed=0, name="hk"):
    """Segments with raw LONG key columns (`a`, and `b` for two-word keys) and a dictionary INT measure `m`: doc d holds
    key row doc_keys[d]; the docs are cut into segments of seg_docs docs (default SEG_DOCS, the last one taking the
    rest). Returns (segments, key rows per doc over all segments [docs] or [docs, 2], measure per doc int64[docs])."""
    from pinot_amd.segment import create_segment
    keys = np.asarray(keys, dtype=np.int64)
    rows = keys[np.asarray(doc_keys, dtype=np.int64)]
    n = len(rows)
    m = np.random.default_rng([seed, n]).integers(MEASURE[0], MEASURE[1], size=n).astype(np.int32)
    if seg_docs is None:
        seg_docs = SEG_DOCS if n > SEG_DOCS[0] else (n,)
    cuts = np.cumsum(seg_docs)[:-1]
    assert n > 0 and (len(cuts) == 0 or cuts[-1] < n)
    two = keys.ndim == 2
    schema = {"a": "LONG", "b": "LONG", "m": "INT"} if two else {"a": "LONG", "m": "INT"}
    segs = []
    for si, (r, mm) in enumerate(zip(np.split(rows, cuts), np.split(m, cuts))):
        data = {"a": np.ascontiguousarray(r[:, 0] if two else r), "m": mm}
        if two:
            data["b"] = np.ascontiguousarray(r[:, 1])
        segs.append(create_segment("%s_%d" % (name, si), data, schema, no_dictionary_columns=("a", "b")))
    return segs, rows, m.astype(np.int64)


def reference(rows, m):
    """{key tuple: [COUNT(*), SUM(m), MIN(m), MAX(m)]} over the docs (key rows, measure): the count an int, the others
    floats holding exact integers, as the engine's intermediate results do."""
    rows = np.asarray(rows, dtype=np.int64)
    m = np.asarray(m, dtype=np.int64)
    uniq, inv = np.unique(rows.reshape(len(rows), -1), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    ng = len(uniq)
    count = np.bincount(inv, minlength=ng)
    total = np.zeros(ng, dtype=np.int64)
    np.add.at(total, inv, m)
    lo = np.full(ng, INT64_MAX, dtype=np.int64)
    hi = np.full(ng, INT64_MIN, dtype=np.int64)
    np.minimum.at(lo, inv, m)
    np.maximum.at(hi, inv, m)
    assert int(np.abs(m).sum()) < 1 << 53
    return {tuple(k): [int(c), float(s), float(a), float(b)]
            for k, c, s, a, b in zip(uniq.tolist(), count.tolist(), total.tolist(), lo.tolist(), hi.tolist())}


def reference_hll(rows, m, log2m):
    """{key tuple: uint8[1 << log2m]}: the HyperLogLog registers of DISTINCTCOUNTHLL(m) per key."""
    from pinot_amd.hll import hash_long, slot_rank
    rows = np.asarray(rows, dtype=np.int64)
    m = np.asarray(m, dtype=np.int64)
    jr = {v: slot_rank(hash_long(v), log2m) for v in np.unique(m).tolist()}
    out = {}
    for k, v in zip(rows.reshape(len(rows), -1).tolist(), m.tolist()):
        regs = out.setdefault(tuple(k), np.zeros(1 << log2m, dtype=np.uint8))
        j, r = jr[v]
        if r > regs[j]:
            regs[j] = r
    return out


def sql(words, aggs="COUNT(*), SUM(m), MIN(m), MAX(m)", tail="LIMIT 1000000"):
    by = "a, b" if words == 2 else "a"
    return "SELECT %s, %s FROM t GROUP BY %s %s" % (by, aggs, by, tail)
