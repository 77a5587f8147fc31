"""tests/hash_keys.py on the CPU: its hash restatements invert and agree with parallel.py's torch ones (which the merge
tests trust), and every key constructor delivers the homes, fingerprints, owners and counts it claims within its
candidate bound."""
import numpy as np
import pytest
import torch

import hash_keys as H
from pinot_amd import parallel as P

MASK = 1023
EDGES = [0, 1, -1, H.INT64_MIN, H.INT64_MAX, 1 << 32, (1 << 33) - 1, (1 << 33) + 1]


def _values():
    rng = np.random.default_rng(11)
    return np.concatenate([np.array(EDGES, dtype=np.int64),
                           rng.integers(H.INT64_MIN, H.INT64_MAX, size=4000, dtype=np.int64, endpoint=True),
                           rng.integers(-(1 << 34), 1 << 34, size=1000, dtype=np.int64)])


def test_mix64_inverts_on_ints_and_arrays():
    v = _values()
    assert np.array_equal(H.signed(H.unmix64(H.mix64(v))), v)
    assert np.array_equal(H.signed(H.mix64(H.unmix64(v))), v)
    for x in v[:300].tolist():
        assert H.signed(H.unmix64(H.mix64(x))) == x and H.signed(H.mix64(H.unmix64(x))) == x
        assert 0 <= H.mix64(x) <= H.M64
    # the Python-int and the numpy forms are one function
    assert [H.mix64(x) for x in v[:300].tolist()] == H.mix64(v[:300]).tolist()
    assert [H.unmix64(x) for x in v[:300].tolist()] == H.unmix64(v[:300]).tolist()
    assert (H.C1 * H.C1_INV) & H.M64 == 1 and (H.C2 * H.C2_INV) & H.M64 == 1


def test_restatements_agree_with_parallel():
    v = _values()
    w = np.roll(v, 7)
    tv, tw = torch.from_numpy(v), torch.from_numpy(w)
    assert np.array_equal(H.signed(H.mix64(v)), P._mix64(tv).numpy())
    for world in (1, 2, 3, 7, 1024):
        assert np.array_equal(H.owner1(v, world), P.key_owner(tv, world).numpy())
        assert np.array_equal(H.owner2(v, w, world), P.key_owner2(tv, tw, world).numpy())
    for a, b in zip(v[:300].tolist(), w[:300].tolist()):
        assert H.owner1(a, 3) == int(P.key_owner(torch.tensor([a]), 3)[0])
        assert H.owner2(a, b, 3) == int(P.key_owner2(torch.tensor([a]), torch.tensor([b]), 3)[0])
    # home and fingerprint: the array and the integer forms agree
    assert [H.home1(x, MASK) for x in v[:300].tolist()] == H.home1(v[:300], MASK).tolist()
    assert [H.home2(a, b, MASK) for a, b in zip(v[:300].tolist(), w[:300].tolist())] == H.home2(v[:300], w[:300], MASK).tolist()
    assert [H.fp2(a, b) for a, b in zip(v[:300].tolist(), w[:300].tolist())] == H.fp2(v[:300], w[:300]).tolist()
    assert int(H.fp2(v, w).max()) <= H.FP_MASK


def _distinct(keys):
    return len(np.unique(keys.reshape(len(keys), -1), axis=0)) == len(keys)


@pytest.mark.parametrize("home,n", [(1023, 1024), (1020, 40), (0, 7)])
def test_chain1(home, n):
    t = H.Tally()
    k = H.chain1(home, n, MASK, tally=t)
    assert k.dtype == np.int64 and k.shape == (n,) and _distinct(k)
    assert (H.home1(k, MASK) == home).all() and not (k == H.INT64_MAX).any()
    assert t.tried <= H.CANDIDATES_PER_KEY * (MASK + 1) * n and t.tried <= n + 1  # (one candidate a key)


def test_chain1_never_yields_the_empty_marker():
    """INT64_MAX is a member of its home slot's chain (some j gives it): the constructor steps over it."""
    home = H.home1(H.INT64_MAX, MASK)
    j = H.mix64(H.INT64_MAX) >> 10
    t = H.Tally()
    k = H.chain1(home, 3, MASK, start=j - 1, tally=t)
    assert t.tried == 4 and not (k == H.INT64_MAX).any() and (H.home1(k, MASK) == home).all()
    assert H.signed(H.unmix64(home + 1024 * j)) == H.INT64_MAX


@pytest.mark.parametrize("home,n", [(1023, 1024), (1022, 9)])
def test_chain2(home, n):
    t = H.Tally()
    k = H.chain2(home, n, MASK, tally=t)
    assert k.dtype == np.int64 and k.shape == (n, 2) and _distinct(k)
    assert (H.home2(k[:, 0], k[:, 1], MASK) == home).all()
    assert len(np.unique(H.fp2(k[:, 0], k[:, 1]))) == n
    assert t.tried <= H.CANDIDATES_PER_KEY * (MASK + 1) * n


def test_fp_collisions():
    base = H.chain2(1019, 1, MASK)[0]
    t = H.Tally()
    k = H.fp_collisions(int(base[0]), int(base[1]), 6, MASK, tally=t)
    both = np.concatenate([base[None, :], k])
    assert k.shape == (6, 2) and k.dtype == np.int64 and _distinct(both)
    assert (H.fp2(both[:, 0], both[:, 1]) == H.fp2(int(base[0]), int(base[1]))).all()
    assert (H.home2(both[:, 0], both[:, 1], MASK) == 1019).all()
    assert t.tried <= H.CANDIDATES_PER_KEY * (MASK + 1) * 6
    # edge-valued base pairs work the same
    k = H.fp_collisions(H.INT64_MAX, H.INT64_MIN, 2, MASK)
    assert (H.fp2(k[:, 0], k[:, 1]) == H.fp2(H.INT64_MAX, H.INT64_MIN)).all()
    assert (H.home2(k[:, 0], k[:, 1], MASK) == H.home2(H.INT64_MAX, H.INT64_MIN, MASK)).all()


@pytest.mark.parametrize("world,rank", [(2, 0), (3, 0), (3, 2)])
def test_owned_by(world, rank):
    t = H.Tally()
    k = H.take(60, H.owned_by(rank, world, H.iter_chain1(1000, MASK, tally=t)), MASK, t)
    assert k.shape == (60,) and _distinct(k) and (H.home1(k, MASK) == 1000).all()
    assert (H.owner1(k, world) == rank).all()
    assert t.tried <= H.CANDIDATES_PER_KEY * (MASK + 1) * 60
    t = H.Tally()
    k = H.take(60, H.owned_by(rank, world, H.iter_chain2(1000, MASK, tally=t)), MASK, t)
    assert k.shape == (60, 2) and _distinct(k) and (H.home2(k[:, 0], k[:, 1], MASK) == 1000).all()
    assert (H.owner2(k[:, 0], k[:, 1], world) == rank).all()
    base = k[0]
    t = H.Tally()
    c = H.take(3, H.owned_by(rank, world, H.iter_fp_collisions(int(base[0]), int(base[1]), MASK, tally=t)), MASK, t)
    assert (H.owner2(c[:, 0], c[:, 1], world) == rank).all()
    assert (H.fp2(c[:, 0], c[:, 1]) == H.fp2(int(base[0]), int(base[1]))).all()
    assert (H.home2(c[:, 0], c[:, 1], MASK) == 1000).all()
    assert t.tried <= H.CANDIDATES_PER_KEY * (MASK + 1) * 3


def test_spread_keys():
    k = H.spread1(1024, 3)
    assert k.shape == (1024,) and _distinct(k) and not (k == H.INT64_MAX).any()
    assert len(np.unique(H.home1(k, MASK))) > 512  # (homes as they fall: most slots' chains are short)
    assert np.array_equal(k, H.spread1(1024, 3))
    p = H.spread2(1027, 4)
    assert p.shape == (1027, 2) and _distinct(p)


def test_a_search_that_finds_nothing_stops():
    """The bound is carried by the candidate stream: a filter no candidate passes raises and does not spin."""
    t = H.Tally()
    with pytest.raises(RuntimeError, match="key search"):
        H.take(1, (k for k in H.iter_chain1(5, MASK, tally=t) if False), MASK, t)
    assert t.tried == H.CANDIDATES_PER_KEY * (MASK + 1) + 1


def test_layout_and_reference():
    mult = np.array([3, 1, 4, 2])
    docs = H.layout(mult, pinned=[(0, 2), (1, 0), (9, 2)], seed=5)
    assert docs[0] == 2 and docs[1] == 0 and docs[9] == 2 and np.array_equal(np.bincount(docs), mult)
    keys = np.array([[5, -1], [5, 0], [H.INT64_MAX, H.INT64_MIN], [-7, 9]], dtype=np.int64)
    segs, rows, m = H.build_segments(keys, docs, seg_docs=(4, 6))
    assert [s.num_docs for s in segs] == [4, 6] and np.array_equal(rows, keys[docs])
    assert np.array_equal(np.concatenate([s.column("a").raw_values for s in segs]), rows[:, 0])
    assert np.array_equal(np.concatenate([s.column("b").raw_values for s in segs]), rows[:, 1])
    assert not segs[0].column("a").has_dictionary and segs[0].column("m").has_dictionary
    ref = H.reference(rows, m)
    assert set(ref) == {tuple(k) for k in keys.tolist()}
    for i, k in enumerate(keys.tolist()):
        mm = m[docs == i]
        assert ref[tuple(k)] == [int(mult[i]), float(mm.sum()), float(mm.min()), float(mm.max())]
    regs = H.reference_hll(rows, m, 8)
    from pinot_amd.hll import HyperLogLog
    for i, k in enumerate(keys.tolist()):
        h = HyperLogLog(8)
        for v in m[docs == i].tolist():
            h.offer(v, "INT")
        assert np.array_equal(h.registers, regs[tuple(k)])
