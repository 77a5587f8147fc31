// Scan strategy: partitioned aggregation, count + emit passes (STRAT_PCOUNT*, the pemit strategies).
// Included by the pa_scan_part_*.hip units in place of pa_scan.h, which declares the entry points it calls and
// includes no strategy.
#pragma once
#include "pa_scan.h"

namespace pa {

// ---------------------------------------------------------------- partitioned aggregation: count + emit passes
// LDS bin state of the emit pass, per partition (V partitions first, then H): records in the bin (may pass the bin
// size while a flush is in progress: the excess goes straight to the range), records written into it, the range's next
// whole-bin slot (front) and its last free record (back), and the range's first record in the stream.
// All of it through address-space-3 pointers: ds_* instructions. A flat access could alias global memory, and waiting
// for one (flat loads count in vmcnt) would drain the tile ring's LDS-DMA.
struct BinState {
  lds_u32_t* cnt;
  lds_u32_t* done;
  lds_u32_t* front;
  lds_u32_t* back;
  lds_u64_t* start;
  lds_u32_t* slk;   // H bins: records of the doc that crossed the bin end, parked past it (<= kDocVals - 1)
};

__device__ __forceinline__ BinState bin_state(const DevQuery* __restrict__ q, unsigned char* lds) {
  return BinState{lds_ptr(lds + q->lds_cnt), lds_ptr(lds + q->lds_done), lds_ptr(lds + q->lds_front),
                  lds_ptr(lds + q->lds_back), (lds_u64_t*)lds_ptr(lds + q->lds_start),
                  lds_ptr(lds + q->lds_slack) - q->pv};  // (slack words exist for the H partitions only)
}

// Wave-level put of K records per lane: every lane calls it (uniform control flow); record k of an active lane (the
// first nw words of r[k]) goes into partition p[k]'s LDS bin of BS records (bins: the stream's partitions from p0 on,
// BS * nw words each). Phases, each a run of independent LDS operations (one wait per phase, not per record):
// claim slots (cnt), write them, count them written (done). The lane whose write completes a bin marks it, and the
// wave then stores every marked bin of the batch at its range's front slot — several bins per store instruction (L
// lanes per bin, one 16-byte unit each) — and empties it; a record whose bin was full claims again after that. Every
// (workgroup, partition) range holds exactly the records the count pass counted, so front and back meet (checked at
// the end of the pass). Without RETRY a record whose bin is full goes to the range's back end instead.
// Ordering: LDS executes the DS instructions of one wave in issue order and serialises those of different waves, so
// "write the slot, then count it done" and "read the bin, then reset the counters" need only the compiler to keep
// program order (a signal fence). Acquire/release atomics would also wait for every outstanding global load, i.e.
// drain the tile ring's LDS-DMA on every record. Only the wave that completed a bin touches its front and counters
// until it resets them (a bin fills at most once per claim round: it stays full until its flush).
template <int K, bool SL = false>
__device__ __forceinline__ void flush_full_bins(const BinState& B, const bool (&full)[K], const uint32_t (&p)[K],
                                                uint32_t p0, lds_u32_t* bins, uint32_t BS, uint32_t nw,
                                                AS1 uint32_t* recs, int lane, int dbg, uint32_t BST = 0);

template <int K, int WM, bool SL = false, bool RETRY = false>
__device__ __forceinline__ void bin_put_batch(const BinState& B, const bool (&act)[K], const uint32_t (&p)[K],
                                              uint32_t p0, lds_u32_t* bins, uint32_t BS, uint32_t nw,
                                              const uint32_t (&r)[K][WM], AS1 uint32_t* recs, int lane, int dbg,
                                              uint32_t BST = 0) {
  if (BST == 0) BST = BS;
  // RETRY (the MV group-by's V records, several per doc: their bins fill fast and the back path's 4-byte stores
  // dominated, r04_c1 -> r04_c3 emit 5.76 -> 4.86 ms) or the back path (one record per doc: the retry rounds cost
  // more than the few scattered stores, configs[2] emit 1.29 -> 1.41 ms, configs[4] V emit 1.5 -> 1.9 ms)
  if constexpr (!RETRY) {
    uint32_t s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = act[k] ? __hip_atomic_fetch_add(B.cnt + p[k], 1u, WG_RLX) : 0xffffffffu;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (s[k] < BS) {
        lds_u32_t* slot = bins + ((p[k] - p0) * BST + s[k]) * nw;
#pragma unroll
        for (int w = 0; w < WM; ++w)
          if ((uint32_t)w < nw) slot[w] = r[k][w];
      }
    }
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    bool full[K];
#pragma unroll
    for (int k = 0; k < K; ++k) full[k] = s[k] < BS && __hip_atomic_fetch_add(B.done + p[k], 1u, WG_RLX) == BS - 1u;
    if (!(dbg & 1)) {  // a record whose bin is full goes straight to the back end of its range
      uint32_t o[K];
#pragma unroll
      for (int k = 0; k < K; ++k)
        o[k] = (act[k] && s[k] >= BS) ? __hip_atomic_fetch_sub(B.back + p[k], 1u, WG_RLX) - 1u : 0u;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        if (act[k] && s[k] >= BS) {
          AS1 uint32_t* d = recs + (B.start[p[k]] + o[k]) * (uint64_t)nw;
#pragma unroll
          for (int w = 0; w < WM; ++w)
            if ((uint32_t)w < nw) d[w] = r[k][w];
        }
      }
    }
    flush_full_bins<K, SL>(B, full, p, p0, bins, BS, nw, recs, lane, dbg, BST);
    return;
  }
  // A record whose bin is full (claimed past BS while its completing wave flushes it) retries after this wave has
  // flushed the bins it completed itself (so no wave waits for a bin whose flusher waits too): every record leaves
  // through a whole-bin burst, never as a scattered store (a 4-byte store costs a whole 64-byte HBM write).
  bool pend[K];
#pragma unroll
  for (int k = 0; k < K; ++k) pend[k] = act[k];
  for (int round = 0;; ++round) {
    uint32_t s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = pend[k] ? __hip_atomic_fetch_add(B.cnt + p[k], 1u, WG_RLX) : 0xffffffffu;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (s[k] < BS) {
        lds_u32_t* slot = bins + ((p[k] - p0) * BST + s[k]) * nw;
#pragma unroll
        for (int w = 0; w < WM; ++w)
          if ((uint32_t)w < nw) slot[w] = r[k][w];
      }
    }
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    bool full[K];
#pragma unroll
    for (int k = 0; k < K; ++k) full[k] = s[k] < BS && __hip_atomic_fetch_add(B.done + p[k], 1u, WG_RLX) == BS - 1u;
    flush_full_bins<K, SL>(B, full, p, p0, bins, BS, nw, recs, lane, dbg, BST);
    bool any = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      pend[k] = pend[k] && s[k] >= BS;
      any |= pend[k];
    }
    if (__ballot(any) == 0) break;
    if (round > 0) __builtin_amdgcn_s_sleep(2);  // (the bin's flush is a few hundred cycles away)
  }
}

// The flush half of a put: every bin some lane completed (full[k]) is stored at its range's front slot — several bins
// per store instruction (L lanes per bin, one 16-byte unit each) — and emptied.
// SL (H bins of the doc-reserved path): bins are BST records apart and may hold a crossing doc's tail past BS
// (B.slk); after the store it moves to the bin's front and the bin restarts with it.
template <int K, bool SL>
__device__ __forceinline__ void flush_full_bins(const BinState& B, const bool (&full)[K], const uint32_t (&p)[K],
                                                uint32_t p0, lds_u32_t* bins, uint32_t BS, uint32_t nw,
                                                AS1 uint32_t* recs, int lane, int dbg, uint32_t BST) {
  if (BST == 0) BST = BS;
  uint64_t fm[K];
  uint64_t any = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    fm[k] = __ballot(full[k]);
    any |= fm[k];
  }
  if (any == 0) return;
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  if (dbg & 1) {  // (measurement only: drop the bins)
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (full[k]) {
        const uint32_t r = SL ? B.slk[p[k]] : 0u;
        if (SL) B.slk[p[k]] = 0u;
        __hip_atomic_store(B.done + p[k], r, WG_RLX);
        __hip_atomic_store(B.cnt + p[k], r, WG_RLX);
      }
    }
    return;
  }
  // L lanes per bin (the bin's 16-byte units, rounded up to a power of two), G = 64 / L bins per store round
  const uint32_t n16 = (BS * nw) >> 2;
  uint32_t L = 1;
  while (L < n16 && L < (uint32_t)kWave) L <<= 1;
  const uint32_t G = (uint32_t)kWave / L;
  const uint32_t grp = (uint32_t)lane / L, c0 = (uint32_t)lane % L;
  uint32_t mine = 0xffffffffu, g = 0;
  auto store_round = [&]() {
    const bool on = grp < g;
    uint32_t o = 0, r = 0;
    if (on) {
      o = B.front[mine];
      AS1 u32x4* d = (AS1 u32x4*)(recs + (B.start[mine] + o) * (uint64_t)nw);
      const lds_u32x4_t* sb = (const lds_u32x4_t*)(bins + (mine - p0) * BST * nw);
      for (uint32_t c = c0; c < n16; c += L) d[c] = sb[c];
    }
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    if (SL && on) {  // the parked tail (one record per lane, nw == 1) to the bin's front
      r = B.slk[mine];
      lds_u32_t* b1 = bins + (mine - p0) * BST;
      for (uint32_t c = c0; c < r; c += L) b1[c] = b1[BS + c];  // (r < kDocVals; L may be smaller)
    }
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    if (on && c0 == 0) {
      B.front[mine] = o + BS;
      if (SL) B.slk[mine] = 0u;
      __hip_atomic_store(B.done + mine, r, WG_RLX);
      __hip_atomic_store(B.cnt + mine, r, WG_RLX);
    }
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    g = 0;
    mine = 0xffffffffu;
  };
#pragma unroll
  for (int k = 0; k < K; ++k) {
    uint64_t m = fm[k];
    while (m) {
      const int l = __builtin_ctzll(m);
      m &= m - 1;
      const uint32_t pp = (uint32_t)__builtin_amdgcn_readlane((int)p[k], l);
      if (grp == g) mine = pp;
      if (++g == G) store_round();
    }
  }
  if (g) store_round();
}

// One record per lane (K = 1).
template <int WM>
__device__ __forceinline__ void bin_put_wave(const BinState& B, bool active, uint32_t p, uint32_t p0, lds_u32_t* bins,
                                             uint32_t BS, uint32_t nw, const uint32_t (&r)[WM], AS1 uint32_t* recs,
                                             int lane, int dbg) {
  const bool a[1] = {active};
  const uint32_t pk[1] = {p};
  uint32_t rr[1][WM];
#pragma unroll
  for (int w = 0; w < WM; ++w) rr[0][w] = r[w];
  bin_put_batch<1, WM>(B, a, pk, p0, bins, BS, nw, rr, recs, lane, dbg);
}


// MV value range [v0, v1) of the matching docs of steps h .. h+N-1 (0, 0 elsewhere, or without an MV column); nd =
// the segment's docs (hoff holds nd + 1 offsets).
template <int N, int LM>
__device__ __forceinline__ void mv_ranges(bool hmv, const int32_t* hoff, int64_t nd, int64_t doc_base, int h, uint32_t m,
                                          int lane, int32_t (&v0)[N], int32_t (&v1)[N]) {
  auto local = [&](int i) { return LM ? 32 * lane + i : i * kWave + lane; };
  if constexpr (!LM) {
    // step i holds docs doc_base + 64 i + lane: a doc's end offset is the next lane's start offset, so one coalesced
    // load per step (every doc of the step, clamped to nd) plus lane 63's end offset
    int32_t a[N], b[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      a[i] = b[i] = 0;
      if (hmv) {
        const int64_t doc = doc_base + local(h + i);
        a[i] = gp(hoff)[doc < nd ? doc : nd];
        if (lane == kWave - 1) b[i] = gp(hoff)[doc + 1 < nd ? doc + 1 : nd];
      }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int32_t nx = __shfl_down(a[i], 1, kWave);
      const bool on = hmv && ((m >> (h + i)) & 1u);
      v0[i] = on ? a[i] : 0;
      v1[i] = on ? (lane == kWave - 1 ? b[i] : nx) : 0;
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      v0[i] = v1[i] = 0;
      if (hmv && ((m >> (h + i)) & 1u)) {
        const int64_t doc = doc_base + local(h + i);
        v0[i] = gp(hoff)[doc];
        v1[i] = gp(hoff)[doc + 1];
      }
    }
  }
}


// Table-wide keys (< 2^32 on the partitioned path) of the docs of steps h .. h+N-1 (match bits m): every group-by
// dictId decode, then every remap gather (they overlap), then the keys.
template <int N, int LM>
__device__ __forceinline__ void part_keys(const DevQuery* __restrict__ q, CSegT* cs, const uint32_t* img,
                                          int64_t doc_base, int h, uint32_t m, int lane, uint32_t (&key)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) key[i] = 0u;
  for (int j = 0; j < q->num_gb; ++j) {
    // (the multi-value component: per value, mv_key_records; the count pass's skipped component: below the partition)
    if (j == q->gb_mv || j == q->count_skip_gb) continue;
    const int slot = q->gb_slot[j];
    const int gl = cs->cols[slot].lds_off, gn = cs->cols[slot].nbits;
    const uint32_t* gw = cs->cols[slot].words;
    const int32_t* rm = cs->remap[j];
    const uint32_t st = (uint32_t)q->gb_stride[j];
    uint32_t id[N];
    decode_batch<N, LM>(gl, gn, gw, img, doc_base, h, m, lane, id);
    if (rm != nullptr) {
#pragma unroll
      for (int i = 0; i < N; ++i)
        if ((m >> (h + i)) & 1u) id[i] = (uint32_t)gp(rm)[id[i]];
    }
#pragma unroll
    for (int i = 0; i < N; ++i) key[i] += id[i] * st;
  }
}

// The V records of one step of a query grouping by a multi-value column (DictionaryBasedGroupKeyGenerator
// .getIntRawKeys: one key per value of the doc's MV group-by column, duplicates included; a doc without values has no
// key). Lane l holds its doc's key without the MV component (`base`), its first value's index v0 and its value count n
// (0: not matching); `adm` (numGroupsLimit walk form, else null) drops the keys the segment did not admit. Value-parallel, KB x 64 records per round: lane j takes record g = b + 64 k + j, finds the owner
// lane (the first whose inclusive prefix sum of n exceeds g) by a 6-shuffle binary search and decodes that value
// (consecutive records are consecutive values of the stream: the loads coalesce). f(act, key, owner) takes each round.
template <int KB, class F>
__device__ __forceinline__ void mv_key_records(const uint32_t* words, int nb, const int32_t* rm, uint32_t stride,
                                               const uint32_t* adm, uint32_t base, int32_t v0, uint32_t n, int lane,
                                               F&& f) {
  uint32_t incl = n;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const uint32_t t = __shfl_up(incl, o, kWave);
    if (lane >= o) incl += t;
  }
  const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);
#pragma unroll 1
  for (uint32_t b = 0; b < total; b += KB * kWave) {
    bool act[KB];
    uint32_t key[KB], id[KB];
    int own[KB];
    int64_t vi[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      const uint32_t g = b + (uint32_t)(k * kWave + lane);
      int ow = 0;
#pragma unroll
      for (int st = kWave / 2; st >= 1; st >>= 1) {
        const uint32_t v = (uint32_t)__shfl((int)incl, ow + st - 1, kWave);
        if (v <= g) ow += st;
      }
      ow = ow < kWave ? ow : kWave - 1;
      const uint32_t o_incl = (uint32_t)__shfl((int)incl, ow, kWave), o_n = (uint32_t)__shfl((int)n, ow, kWave);
      act[k] = g < total;
      own[k] = ow;
      key[k] = (uint32_t)__shfl((int)base, ow, kWave);
      vi[k] = (int64_t)__shfl(v0, ow, kWave) + (int64_t)(g - (o_incl - o_n));
    }
    decode_global_batch<KB>(words, vi, act, nb, id);
    if (rm != nullptr) {
#pragma unroll
      for (int k = 0; k < KB; ++k)
        if (act[k]) id[k] = (uint32_t)gp(rm)[id[k]];
    }
#pragma unroll
    for (int k = 0; k < KB; ++k) key[k] += id[k] * stride;
    if (adm != nullptr) {  // numGroupsLimit, walk form: the keys the segment admitted
      uint32_t w[KB];
#pragma unroll
      for (int k = 0; k < KB; ++k) w[k] = act[k] ? gp(adm)[key[k] >> 5] : 0u;
#pragma unroll
      for (int k = 0; k < KB; ++k) act[k] = act[k] && ((w[k] >> (key[k] & 31u)) & 1u);
    }
    f(act, key, own);
  }
}

// The same records, each lane its own doc (every doc of the step has at most kDocVals values): all of a doc's values
// decoded in one batch (the step's docs are consecutive, so their values are one short stretch of the stream and the
// loads nearly coalesce), no cross-lane shuffles; f(act, key) takes all of them (act[e]: value e exists and is
// admitted).
template <class F>
__device__ __forceinline__ void mv_doc_records(const uint32_t* words, int nb, const int32_t* rm, uint32_t stride,
                                               const uint32_t* adm, uint32_t base, int32_t v0, uint32_t n,
                                               uint32_t maxn, F&& f) {
  uint32_t id[kDocVals], key[kDocVals];
  int64_t vi[kDocVals];
  bool on[kDocVals];
#pragma unroll
  for (int e = 0; e < kDocVals; ++e) {
    vi[e] = (int64_t)v0 + e;
    on[e] = (uint32_t)e < n;
  }
  decode_global_batch<kDocVals>(words, vi, on, nb, id);
  if (rm != nullptr) {
#pragma unroll
    for (int e = 0; e < kDocVals; ++e)
      if (on[e]) id[e] = (uint32_t)gp(rm)[id[e]];
  }
#pragma unroll
  for (int e = 0; e < kDocVals; ++e) key[e] = base + id[e] * stride;
  if (adm != nullptr) {
    uint32_t w[kDocVals];
#pragma unroll
    for (int e = 0; e < kDocVals; ++e) w[e] = on[e] ? gp(adm)[key[e] >> 5] : 0u;
#pragma unroll
    for (int e = 0; e < kDocVals; ++e) on[e] = on[e] && ((w[e] >> (key[e] & 31u)) & 1u);
  }
  f(on, key);
  (void)maxn;
}

// The V payload of one value column for the docs of steps h .. h+N-1: V_FMT_ID its table-wide value id (lo), V_FMT_32 /
// V_FMT_64 its value bits (lo, hi): a dictionary gather, or the raw value (a raw DOUBLE's bits unchanged).
template <int N, int LM, int VF>
__device__ __forceinline__ void part_vvals(const DevQuery* __restrict__ q, CSegT* cs, const uint32_t* img,
                                           int64_t doc_base, int h, uint32_t m, int lane, uint32_t (&lo)[N],
                                           uint32_t (&hi)[N]) {
  auto local = [&](int i) { return LM ? 32 * lane + i : i * kWave + lane; };
#pragma unroll
  for (int i = 0; i < N; ++i) lo[i] = hi[i] = 0u;
  if constexpr (VF == V_FMT_ID || VF == V_FMT_32 || VF == V_FMT_64) {
    const int va = q->emit_val_agg;
    const int vslot = q->aggs[va].slot;
    const int vkind = cs->cols[vslot].kind;
    const int vl = cs->cols[vslot].lds_off, vn = cs->cols[vslot].nbits, vtype = cs->cols[vslot].vtype;
    const uint32_t* vw = cs->cols[vslot].words;
    const uint64_t* vd = q->aggs[va].src == SRC_DOUBLE ? (const uint64_t*)cs->cols[vslot].dict_f64
                                                        : (const uint64_t*)cs->cols[vslot].dict_i64;
    const int32_t* vrm = cs->vremap;
    const void* vraw = cs->cols[vslot].raw;
    if (vkind == COL_SV_DICT) {
      uint32_t vid[N];
      decode_batch<N, LM>(vl, vn, vw, img, doc_base, h, m, lane, vid);
      if constexpr (VF == V_FMT_ID) {
        if (vrm != nullptr) {
#pragma unroll
          for (int i = 0; i < N; ++i)
            if ((m >> (h + i)) & 1u) vid[i] = (uint32_t)gp(vrm)[vid[i]];
        }
#pragma unroll
        for (int i = 0; i < N; ++i) lo[i] = vid[i];
      } else {
#pragma unroll
        for (int i = 0; i < N; ++i) {
          if (!((m >> (h + i)) & 1u)) continue;
          const uint64_t v = gp(vd)[vid[i]];
          lo[i] = (uint32_t)v;
          hi[i] = (uint32_t)(v >> 32);
        }
      }
    } else if (vtype == PA_INT) {
#pragma unroll
      for (int i = 0; i < N; ++i) {
        if (!((m >> (h + i)) & 1u)) continue;
        lo[i] = (uint32_t)gp((const int32_t*)vraw)[doc_base + local(h + i)];
        hi[i] = (uint32_t)((int32_t)lo[i] >> 31);
      }
    } else {  // LONG, or DOUBLE bits (a SUM/MIN/MAX over a raw DOUBLE column reads the bits unchanged)
#pragma unroll
      for (int i = 0; i < N; ++i) {
        if (!((m >> (h + i)) & 1u)) continue;
        const uint64_t v = gp((const uint64_t*)vraw)[doc_base + local(h + i)];
        lo[i] = (uint32_t)v;
        hi[i] = (uint32_t)(v >> 32);
      }
    }
  }
}

// part_tile of a query grouping by a multi-value column (one V record per (doc, value) pair; V stream only, no
// generic records): the kernel variants STRAT_PCOUNT_MV / pemit_strat(.., mv = 1), so its expansion's registers stay out
// of the SV variants' allocation.
template <int STRAT, int STEPS, int LM>
__device__ __forceinline__ void part_tile_mv(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                          const uint32_t* img, int64_t doc_base, uint32_t m, int lane,
                                          unsigned char* lds, const PartScratch& ps) {
  CSegT* cs = (CSegT*)(uintptr_t)uniform_ptr(seg);
  const int ksv = q->kshift_v;
  const int gmv = q->gb_mv;
  const int mslot = q->gb_slot[gmv];
  const int32_t* moff = cs->cols[mslot].mv_off;
  const uint32_t* mwords = cs->cols[mslot].words;
  const int mnb = cs->cols[mslot].nbits;
  const int32_t* mrm = cs->remap[gmv];
  const uint32_t mstride = (uint32_t)q->gb_stride[gmv];
  constexpr int kEB = 8;
  if constexpr (is_pcount(STRAT) && !LM) {
    // Count pass of GROUP BY <sv>, <mv> whose SV component cannot change a partition (count_skip_gb): a record's
    // partition is (value id * stride) >> shift, so a tile whose docs all match counts its whole value range as one
    // coalesced stream (no per-doc expansion)
    if (gmv >= 0 && q->num_gb == 2 && q->count_skip_gb == 1 - gmv && cs->admit == nullptr) {
      const int64_t nd = (int64_t)cs->num_docs, rem = nd - doc_base;
      uint32_t valid = STEPS == 32 ? 0xffffffffu : ((1u << STEPS) - 1u);
      if (rem < STEPS * kWave) {
        const int64_t n = rem > lane ? (rem - lane + kWave - 1) / kWave : 0;
        valid = n >= 32 ? 0xffffffffu : ((1u << n) - 1u);
      }
      if (__ballot(m != valid) == 0) {
        const int64_t d1 = rem < STEPS * kWave ? nd : doc_base + STEPS * kWave;
        const int64_t vlo = gp(moff)[doc_base], vhi = gp(moff)[d1];
        lds_u32_t* hist = lds_ptr(lds);
        constexpr int kVB = 4;
#pragma unroll 1
        for (int64_t v = vlo; v < vhi; v += kVB * kWave) {
          int64_t vi[kVB];
          bool on[kVB];
          uint32_t id[kVB];
#pragma unroll
          for (int k = 0; k < kVB; ++k) {
            vi[k] = v + k * kWave + lane;
            on[k] = vi[k] < vhi;
          }
          decode_global_batch<kVB>(mwords, vi, on, mnb, id);
          if (mrm != nullptr) {
#pragma unroll
            for (int k = 0; k < kVB; ++k)
              if (on[k]) id[k] = (uint32_t)gp(mrm)[id[k]];
          }
#pragma unroll
          for (int k = 0; k < kVB; ++k)
            if (on[k]) __hip_atomic_fetch_add(hist + ((id[k] * mstride) >> ksv), 1u, WG_RLX);
        }
        return;
      }
    }
  }
#pragma unroll 1
  for (int h = 0; h < STEPS; h += kEB) {
    if (__ballot((m >> h) != 0) == 0) break;
    uint32_t key[kEB];
    part_keys<kEB, LM>(q, cs, img, doc_base, h, m, lane, key);  // (without the MV component)
    if constexpr (is_pcount(STRAT)) {
      lds_u32_t* hist = lds_ptr(lds);
      {  // one V record per (doc, value): count each value's partition
        int32_t v0[kEB], v1[kEB];
        mv_ranges<kEB, LM>(true, moff, (int64_t)cs->num_docs, doc_base, h, m, lane, v0, v1);
        if (q->count_skip_gb == gmv && cs->admit == nullptr) {  // the MV component cannot change the partition
#pragma unroll
          for (int i = 0; i < kEB; ++i)
            if (v1[i] > v0[i]) __hip_atomic_fetch_add(hist + (key[i] >> ksv), (uint32_t)(v1[i] - v0[i]), WG_RLX);
          continue;
        }
#pragma clang loop unroll(full)
        for (int i = 0; i < kEB; ++i) {  // (unrolled: constant register indices)
          if (__ballot((m >> (h + i)) & 1u) == 0) continue;
          const int32_t a0 = pick(v0, i), a1 = pick(v1, i);
          const uint32_t nv = (uint32_t)(a1 - a0), maxn = wave_max_u32(nv);
          if (maxn <= (uint32_t)kDocVals) {
            mv_doc_records(mwords, mnb, mrm, mstride, cs->admit, pick(key, i), a0, nv, maxn,
                           [&](const bool (&act)[kDocVals], const uint32_t (&k)[kDocVals]) {
#pragma unroll
                             for (int e = 0; e < kDocVals; ++e)
                               if (act[e]) __hip_atomic_fetch_add(hist + (k[e] >> ksv), 1u, WG_RLX);
                           });
            continue;
          }
          mv_key_records<4>(mwords, mnb, mrm, mstride, cs->admit, pick(key, i), a0, nv, lane,
                            [&](const bool (&act)[4], const uint32_t (&k)[4], const int (&)[4]) {
#pragma unroll
                              for (int kk = 0; kk < 4; ++kk)
                                if (act[kk]) __hip_atomic_fetch_add(hist + (k[kk] >> ksv), 1u, WG_RLX);
                            });
        }
        continue;
      }
    } else {
      constexpr int VF = pemit_vf(STRAT);
      constexpr int NW = VF == V_FMT_32 ? 2 : (VF == V_FMT_64 ? 3 : 1);
      const BinState B = bin_state(q, lds);
      const int dbg = q->debug_emit;
      const uint32_t W = (uint32_t)NW;
      const uint32_t BS = (uint32_t)q->bs_v;
      lds_u32_t* bins = lds_ptr(lds + q->lds_bins_v);
      const uint32_t kmask = (1u << ksv) - 1u;
      uint32_t lo[kEB], hi[kEB];
      part_vvals<kEB, LM, VF>(q, cs, img, doc_base, h, m, lane, lo, hi);
          {  // one record per (doc, value) pair, the doc's payload on each
            int32_t v0[kEB], v1[kEB];
            mv_ranges<kEB, LM>(true, moff, (int64_t)cs->num_docs, doc_base, h, m, lane, v0, v1);
#pragma clang loop unroll(full)
            for (int i = 0; i < kEB; ++i) {  // (unrolled: constant register indices)
              if (__ballot((m >> (h + i)) & 1u) == 0) continue;
              const int32_t a0 = pick(v0, i), a1 = pick(v1, i);
              const uint32_t dlo = pick(lo, i), dhi = pick(hi, i);
              const uint32_t nv = (uint32_t)(a1 - a0), maxn = wave_max_u32(nv);
              // each record: key offset (| value id), the doc's payload
              auto rec = [&](uint32_t k, uint32_t plo, uint32_t phi, uint32_t (&r)[NW]) {
                r[0] = k & kmask;
#pragma unroll
                for (int w = 1; w < NW; ++w) r[w] = 0u;
                if constexpr (VF == V_FMT_ID) {
                  r[0] |= plo << ksv;
                } else if constexpr (VF == V_FMT_32) {
                  r[1] = plo;
                } else if constexpr (VF == V_FMT_64) {
                  r[1] = plo;
                  r[2] = phi;
                }
              };
              if (maxn <= (uint32_t)kDocVals) {  // each lane its own doc's records, all in one put (one wait per phase)
                mv_doc_records(mwords, mnb, mrm, mstride, cs->admit, pick(key, i), a0, nv, maxn,
                               [&](const bool (&act)[kDocVals], const uint32_t (&k)[kDocVals]) {
                                 uint32_t pk[kDocVals], r[kDocVals][NW];
#pragma unroll
                                 for (int e = 0; e < kDocVals; ++e) {
                                   pk[e] = k[e] >> ksv;
                                   rec(k[e], dlo, dhi, r[e]);
                                 }
                                 bin_put_batch<kDocVals, NW, false, true>(B, act, pk, 0u, bins, BS, W, r, gp(ps.recs_v),
                                                                          lane, dbg);
                               });
                continue;
              }
              mv_key_records<4>(mwords, mnb, mrm, mstride, cs->admit, pick(key, i), a0, nv, lane,
                                [&](const bool (&act)[4], const uint32_t (&k)[4], const int (&own)[4]) {
                                  uint32_t pk[4], r[4][NW];
#pragma unroll
                                  for (int kk = 0; kk < 4; ++kk) {
                                    const uint32_t olo = (uint32_t)__shfl((int)dlo, own[kk], kWave);
                                    pk[kk] = k[kk] >> ksv;
                                    r[kk][0] = k[kk] & kmask;
#pragma unroll
                                    for (int w = 1; w < NW; ++w) r[kk][w] = 0u;
                                    if constexpr (VF == V_FMT_ID) {
                                      r[kk][0] |= olo << ksv;
                                    } else if constexpr (VF == V_FMT_32) {
                                      r[kk][1] = olo;
                                    } else if constexpr (VF == V_FMT_64) {
                                      r[kk][1] = olo;
                                      r[kk][2] = (uint32_t)__shfl((int)dhi, own[kk], kWave);
                                    }
                                  }
                                  bin_put_batch<4, NW, false, true>(B, act, pk, 0u, bins, BS, W, r, gp(ps.recs_v), lane,
                                                                    dbg);
                                });
            }
            continue;
          }
    }
  }
}

// The matching docs of one tile (match words m) in the count pass (STRAT_PCOUNT: per (workgroup, partition) record
// counts in LDS) or the emit pass (STRAT_PEMIT: the records into the partition bins). Per batch of 8 steps: every
// group-by dictId decode, then every remap gather (they overlap), then the table-wide keys; then per stream.
template <int STRAT, int STEPS, int LM>
__device__ __forceinline__ void part_tile(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                          const uint32_t* img, int64_t doc_base, uint32_t m, int lane,
                                          unsigned char* lds, const PartScratch& ps) {
  // Descriptors through the constant address space: the segment is read-only during the kernel and its pointer is
  // wave-uniform, so every field is a scalar load the compiler keeps across the LDS atomics and the record stores.
  CSegT* cs = (CSegT*)(uintptr_t)seg;
  auto local = [&](int i) { return LM ? 32 * lane + i : i * kWave + lane; };
  const int pv = q->pv;
  const int ksv = q->kshift_v, ksh = q->kshift_h;
  const int ha = q->hll_agg;
  const int hslot = ha >= 0 ? q->aggs[ha].slot : 0;
  const bool hmv = ha >= 0 && cs->cols[hslot].kind == COL_MV_DICT;
  const int32_t* hoff = cs->cols[hslot].mv_off;
  // steps per batch (register budget; 4 for the H-only emit measured slower: 4.83 vs 4.65 ms). The V-only emit of
  // 4-wave workgroups runs at most 2 workgroups per CU (its LDS bins), so it has the VGPRs for a whole tile per batch.
  constexpr int kEB = (is_pemit(STRAT) && !pemit_hh(STRAT) && !pemit_big(STRAT) && pemit_vf(STRAT) != V_FMT_GEN) ? 16 : 8;
  if constexpr (part_mv(STRAT)) {
    part_tile_mv<STRAT, STEPS, LM>(q, seg, img, doc_base, m, lane, lds, ps);
    return;
  }
#pragma unroll 1
  for (int h = 0; h < STEPS; h += kEB) {
    if (__ballot((m >> h) != 0) == 0) break;  // wave-uniform: the H records below shuffle across all 64 lanes
    uint32_t key[kEB];
    part_keys<kEB, LM>(q, cs, img, doc_base, h, m, lane, key);  // table-wide key (< 2^32 on this path)
    if constexpr (is_pcount(STRAT)) {
      lds_u32_t* hist = lds_ptr(lds);
      uint32_t n[kEB];
      {
        int32_t v0[kEB], v1[kEB];
        mv_ranges<kEB, LM>(hmv, hoff, (int64_t)cs->num_docs, doc_base, h, m, lane, v0, v1);
#pragma unroll
        for (int i = 0; i < kEB; ++i) n[i] = v1[i] - v0[i] > 0 ? (uint32_t)(v1[i] - v0[i]) : 1u;
      }
#pragma unroll
      for (int i = 0; i < kEB; ++i) {
        if (!((m >> (h + i)) & 1u)) continue;
        if (pv) __hip_atomic_fetch_add(hist + (key[i] >> ksv), 1u, WG_RLX);
        if (ha >= 0) __hip_atomic_fetch_add(hist + pv + (key[i] >> ksh), n[i], WG_RLX);
      }
    } else {
      constexpr int VF = pemit_vf(STRAT);
      const BinState B = bin_state(q, lds);
      const int dbg = q->debug_emit;
      if constexpr (VF >= 0) {
        // V records: the value (or its table-wide value id) of the one payload column, batched like the keys
        constexpr int NW = VF == V_FMT_GEN ? kMaxVWords : (VF == V_FMT_32 ? 2 : (VF == V_FMT_64 ? 3 : 1));
        const uint32_t W = VF == V_FMT_GEN ? (uint32_t)q->rec_words_v : (uint32_t)NW;
        const uint32_t BS = (uint32_t)q->bs_v;
        lds_u32_t* bins = lds_ptr(lds + q->lds_bins_v);
        const uint32_t kmask = (1u << ksv) - 1u;
        uint32_t lo[kEB], hi[kEB];
        part_vvals<kEB, LM, VF>(q, cs, img, doc_base, h, m, lane, lo, hi);
        if constexpr (VF != V_FMT_GEN) {
          // the batch's records (one per matching doc of the kEB steps) in one put: every LDS phase runs once
          bool act[kEB];
          uint32_t pk[kEB], r[kEB][NW];
#pragma unroll
          for (int i = 0; i < kEB; ++i) {
            act[i] = (m >> (h + i)) & 1u;
            pk[i] = key[i] >> ksv;
            r[i][0] = key[i] & kmask;
#pragma unroll
            for (int w = 1; w < NW; ++w) r[i][w] = 0u;
            if constexpr (VF == V_FMT_ID) {
              r[i][0] |= lo[i] << ksv;
            } else if constexpr (VF == V_FMT_32) {
              r[i][1] = lo[i];
            } else if constexpr (VF == V_FMT_64) {
              r[i][1] = lo[i];
              r[i][2] = hi[i];
            }
          }
          bin_put_batch<kEB, NW>(B, act, pk, 0u, bins, BS, W, r, gp(ps.recs_v), lane, dbg);
        }
        if constexpr (VF == V_FMT_GEN) {  // every payload of the record (one put per step: up to kMaxVWords words)
#pragma unroll
        for (int i = 0; i < kEB; ++i) {
          const bool mine = (m >> (h + i)) & 1u;
          if (__ballot(mine) == 0) continue;
          const uint32_t p = key[i] >> ksv;
          uint32_t r[NW];
          r[0] = key[i] & kmask;
#pragma unroll
          for (int w = 1; w < NW; ++w) r[w] = 0u;
          {
            if (mine) {
              const int dl = local(h + i);
              const int64_t doc = doc_base + dl;
              for (int a = 0; a < q->num_aggs; ++a) {
                const DevAgg& A = q->aggs[a];
                if (A.type == PA_AGG_COUNT || a == ha) continue;
                const AggValue v = agg_value(A, a, seg, img, dl, doc);
                const int po = A.pay_off;
                if (A.src == SRC_INT) {
                  if (po < kMaxVWords) r[po] = (uint32_t)v.i;
                } else {
                  const int64_t b = A.src == SRC_DOUBLE ? __builtin_bit_cast(int64_t, v.d) : v.i;
                  if (po + 1 < kMaxVWords) {
                    r[po] = (uint32_t)b;
                    r[po + 1] = (uint32_t)(b >> 32);
                  }
                }
              }
            }
          }
          bin_put_wave<NW>(B, mine, p, 0u, bins, BS, W, r, gp(ps.recs_v), lane, dbg);
        }
        }
      }
      if constexpr (pemit_hh(STRAT)) {
        // H records, value-parallel per step: each matching lane's doc owns n = max(1, values) consecutive records of
        // the step; lane j takes record g = b + j, finds its owner by a 6-shuffle binary search over the inclusive
        // prefix sums of n, and decodes that value (coalesced MV reads, no per-lane loop over a doc's values)
        const DevAgg& H = q->aggs[ha];
        const uint32_t* hwords = cs->cols[hslot].words;
        const int hnb = cs->cols[hslot].nbits;
        const uint32_t* hlut = cs->hll_lut[ha];  // dictId -> (register << 8) | rank
        const uint32_t BS = (uint32_t)q->bs_h;
        const uint32_t BST = BS + (uint32_t)kDocVals;  // bin stride: room for a crossing doc's tail
        lds_u32_t* bins = lds_ptr(lds + q->lds_bins_h);
        const uint32_t kmask = (1u << ksh) - 1u;
        const int fsh = H.log2m + 6;
        const uint32_t first_bit = q->h_first ? 1u : 0u;
        // every step's value ranges first (one wait for the batch)
        int32_t v0s[kEB], nvs[kEB];
        mv_ranges<kEB, LM>(hmv, hoff, (int64_t)cs->num_docs, doc_base, h, m, lane, v0s, nvs);
#pragma unroll
        for (int i = 0; i < kEB; ++i) nvs[i] -= v0s[i];
        // Doc-reserved batch path (every matching doc of the batch has at most kDocVals records), kHS steps at a time
        // with every phase a run of independent operations (one wait per phase): reserve each doc's consecutive bin
        // slots (one cnt atomic per doc; records past the bin's end are reserved at the back of the range), decode
        // every value of every doc (each lane its own docs: the step's docs are consecutive, so their values are one
        // short stretch of the MV stream and the loads stay nearly coalesced), gather their (register, rank), write
        // the records, count them done (one atomic per doc), store the bins that filled.
        bool big = false;
#pragma unroll
        for (int i = 0; i < kEB; ++i) big |= ((m >> (h + i)) & 1u) && nvs[i] > kDocVals;
        if (hmv && __ballot(big) == 0) {
          constexpr int kHS = 2;
#pragma unroll
          for (int h2 = 0; h2 < kEB; h2 += kHS) {
            bool mn[kHS];
            uint32_t nn[kHS], pp[kHS], sl[kHS], inb[kHS], db[kHS];
            uint32_t maxn = 0;
#pragma unroll
            for (int j = 0; j < kHS; ++j) {
              const int i = h2 + j;
              mn[j] = (m >> (h + i)) & 1u;
              nn[j] = mn[j] ? (nvs[i] > 0 ? (uint32_t)nvs[i] : 1u) : 0u;
              maxn = max(maxn, nn[j]);
              pp[j] = (uint32_t)pv + (key[i] >> ksh);
            }
#pragma unroll
            for (int o = 1; o < kWave; o <<= 1) maxn = max(maxn, (uint32_t)__shfl_xor((int)maxn, o, kWave));
            maxn = (uint32_t)__builtin_amdgcn_readfirstlane((int)maxn);
            if (maxn == 0) continue;
#pragma unroll
            for (int j = 0; j < kHS; ++j) sl[j] = mn[j] ? __hip_atomic_fetch_add(B.cnt + pp[j], nn[j], WG_RLX) : 0u;
            // a doc whose slot lies in the bin keeps all its records there (a tail past BS parks in the slack); a doc
            // arriving while the bin is full goes to the back of the range whole
            bool bk[kHS];
#pragma unroll
            for (int j = 0; j < kHS; ++j) {
              bk[j] = mn[j] && sl[j] >= BS;
              inb[j] = (mn[j] && sl[j] < BS) ? min(nn[j], BS - sl[j]) : 0u;
              db[j] = (bk[j] && !(dbg & 1)) ? __hip_atomic_fetch_sub(B.back + pp[j], nn[j], WG_RLX) - nn[j] : 0u;
            }
            uint32_t val[kHS][kDocVals];
#pragma unroll
            for (int j = 0; j < kHS; ++j) {
              int64_t vi[kDocVals];
              bool von[kDocVals];
#pragma unroll
              for (int e = 0; e < kDocVals; ++e) {
                vi[e] = (int64_t)v0s[h2 + j] + e;
                von[e] = (uint32_t)e < maxn && e < nvs[h2 + j] && mn[j];
              }
              if (dbg & 4) {
#pragma unroll
                for (int e = 0; e < kDocVals; ++e) val[j][e] = von[e] ? (uint32_t)e : 0u;
              } else {
                decode_global_batch<kDocVals>(hwords, vi, von, hnb, val[j]);
              }
            }
#pragma unroll
            for (int j = 0; j < kHS; ++j)
#pragma unroll
              for (int e = 0; e < kDocVals; ++e)
                if ((uint32_t)e < maxn && e < nvs[h2 + j] && mn[j] && !(dbg & 2)) val[j][e] = gp(hlut)[val[j][e]];
#pragma unroll
            for (int j = 0; j < kHS; ++j) {
              const uint32_t w = (key[h2 + j] & kmask) << fsh;
              lds_u32_t* bin = bins + (pp[j] - (uint32_t)pv) * BST + sl[j];
              AS1 uint32_t* dd = gp(ps.recs_h) + (B.start[pp[j]] + db[j]);
#pragma unroll
              for (int e = 0; e < kDocVals; ++e) {
                if ((uint32_t)e >= maxn || (uint32_t)e >= nn[j]) continue;
                // (an empty doc's one record has rank 0: no register update; it carries the first-value flag)
                const uint32_t hv = e < nvs[h2 + j] ? val[j][e] : 0u;
                const uint32_t r = w | (e == 0 ? first_bit : 0u) | ((hv >> 8) << 6) | ((hv & 0xffu) << 1);
                if (!bk[j]) bin[e] = r;
                else if (!(dbg & 1)) dd[e] = r;
              }
              if (inb[j] && inb[j] < nn[j]) B.slk[pp[j]] = nn[j] - inb[j];  // the crossing doc's parked tail
            }
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            bool full[kHS];
#pragma unroll
            for (int j = 0; j < kHS; ++j)
              full[j] = inb[j] > 0 && __hip_atomic_fetch_add(B.done + pp[j], inb[j], WG_RLX) + inb[j] == BS;
            flush_full_bins<kHS, true>(B, full, pp, (uint32_t)pv, bins, BS, 1u, gp(ps.recs_h), lane, dbg, BST);
          }
          continue;  // (the batch loop `h`)
        }
#pragma unroll 1
        for (int i = 0; i < kEB; ++i) {
          const bool mine = (m >> (h + i)) & 1u;
          if (__ballot(mine) == 0) continue;
          const int dl = local(h + i);
          const int64_t doc = doc_base + dl;
          uint32_t n = 0, hv_sv = 0;
          const int32_t v0 = v0s[i], nv = nvs[i];
          if (mine) {
            if (hmv) {
              n = nv > 0 ? (uint32_t)nv : 1u;
            } else {
              n = 1u;
              hv_sv = (uint32_t)agg_value(H, ha, seg, img, dl, doc).i;
            }
          }
          if (__ballot(n > (uint32_t)kDocVals) == 0) {
            // Doc-reserved path (every doc of the step has at most kDocVals records): one slot reservation per doc
            // (its records are consecutive in its bin), each lane decodes its own doc's values (the step's docs are
            // consecutive, so their values are one short stretch of the MV stream: the loads stay nearly coalesced),
            // one done count per doc. Records past the bin's end go to the back of the range.
            uint32_t maxn = n;
#pragma unroll
            for (int o = 1; o < kWave; o <<= 1) maxn = max(maxn, (uint32_t)__shfl_xor((int)maxn, o, kWave));
            maxn = (uint32_t)__builtin_amdgcn_readfirstlane((int)maxn);
            const uint32_t kk = key[i];
            const uint32_t p = (uint32_t)pv + (kk >> ksh);
            const uint32_t sl = mine ? __hip_atomic_fetch_add(B.cnt + p, n, WG_RLX) : 0u;
            const uint32_t inbin = (mine && sl < BS) ? min(n, BS - sl) : 0u;
            const bool bk = mine && sl >= BS;  // (see the batched path: a tail past BS parks in the slack)
            uint32_t db = 0;
            if (bk && !(dbg & 1)) db = __hip_atomic_fetch_sub(B.back + p, n, WG_RLX) - n;
            uint32_t hvv[kDocVals];
            if (hmv) {
              uint32_t idv[kDocVals];
              int64_t vi[kDocVals];
              bool von[kDocVals];
#pragma unroll
              for (int e = 0; e < kDocVals; ++e) {
                vi[e] = (int64_t)v0 + e;
                von[e] = (uint32_t)e < maxn && mine && e < nv;
              }
              if (dbg & 4) {
#pragma unroll
                for (int e = 0; e < kDocVals; ++e) idv[e] = von[e] ? (uint32_t)e : 0u;
              } else {
                decode_global_batch<kDocVals>(hwords, vi, von, hnb, idv);
              }
#pragma unroll
              for (int e = 0; e < kDocVals; ++e) {
                hvv[e] = 0u;  // (an empty doc's one record: rank 0, no register update)
                if ((uint32_t)e < maxn && mine && e < nv) hvv[e] = (dbg & 2) ? idv[e] : gp(hlut)[idv[e]];
              }
            } else {
#pragma unroll
              for (int e = 0; e < kDocVals; ++e) hvv[e] = hv_sv;
            }
            const uint32_t w = (kk & kmask) << fsh;
            lds_u32_t* bin = bins + (p - (uint32_t)pv) * BST + sl;
            AS1 uint32_t* dd = gp(ps.recs_h) + (B.start[p] + db);
#pragma unroll
            for (int e = 0; e < kDocVals; ++e) {
              if ((uint32_t)e >= maxn || !mine || (uint32_t)e >= n) continue;
              const uint32_t r = w | (e == 0 ? first_bit : 0u) | ((hvv[e] >> 8) << 6) | ((hvv[e] & 0xffu) << 1);
              if (!bk) bin[e] = r;
              else if (!(dbg & 1)) dd[e] = r;
            }
            if (inbin && inbin < n) B.slk[p] = n - inbin;
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            bool full[1] = {inbin > 0 && __hip_atomic_fetch_add(B.done + p, inbin, WG_RLX) + inbin == BS};
            const uint32_t pa[1] = {p};
            flush_full_bins<1, true>(B, full, pa, (uint32_t)pv, bins, BS, 1u, gp(ps.recs_h), lane, dbg, BST);
            continue;
          }
          uint32_t incl = n;
#pragma unroll
          for (int o = 1; o < kWave; o <<= 1) {
            const uint32_t t = __shfl_up(incl, o, kWave);
            if (lane >= o) incl += t;
          }
          const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);
          const uint32_t kk = key[i];
          constexpr int kHB = 4;  // record chunks of 64 per round: their loads overlap
          for (uint32_t b = 0; b < total; b += kHB * kWave) {
            uint32_t w0[kHB], id[kHB], pk[kHB], alt[kHB];
            int32_t ok[kHB];
            int64_t vi[kHB];
            bool von[kHB];
#pragma unroll
            for (int k = 0; k < kHB; ++k) {
              const uint32_t g = b + (uint32_t)(k * kWave + lane);
              int ow = 0;  // owner lane: the first lane whose inclusive prefix exceeds g
#pragma unroll
              for (int st = kWave / 2; st >= 1; st >>= 1) {
                const uint32_t v = (uint32_t)__shfl((int)incl, ow + st - 1, kWave);
                if (v <= g) ow += st;
              }
              ow = ow < kWave ? ow : kWave - 1;
              const uint32_t o_incl = (uint32_t)__shfl((int)incl, ow, kWave), o_n = (uint32_t)__shfl((int)n, ow, kWave);
              const uint32_t o_key = (uint32_t)__shfl((int)kk, ow, kWave);
              const int32_t o_v0 = __shfl(v0, ow, kWave), o_nv = __shfl(nv, ow, kWave);
              const uint32_t o_hv = (uint32_t)__shfl((int)hv_sv, ow, kWave);
              const uint32_t e = g - (o_incl - o_n);
              ok[k] = g < total ? (hmv ? ((int32_t)e < o_nv ? 2 : 1) : 1) : 0;  // 2: an MV value to look up
              pk[k] = o_key >> ksh;
              w0[k] = ((o_key & kmask) << fsh) | (e == 0 ? first_bit : 0u);
              vi[k] = (int64_t)o_v0 + e;
              von[k] = ok[k] == 2 && !(dbg & 4);
              alt[k] = ok[k] == 2 ? e : (hmv ? 0u : o_hv);  // (e: measurement only, tuning debug_emit bit 2)
            }
            decode_global_batch<kHB>(hwords, vi, von, hnb, id);
#pragma unroll
            for (int k = 0; k < kHB; ++k)
              if (!von[k]) id[k] = alt[k];
            uint32_t hv[kHB];
#pragma unroll
            for (int k = 0; k < kHB; ++k) hv[k] = ok[k] == 2 && !(dbg & 2) ? gp(hlut)[id[k]] : id[k];  // (register << 8) | rank
            bool act[kHB];
            uint32_t pp[kHB], r[kHB][1];
#pragma unroll
            for (int k = 0; k < kHB; ++k) {
              act[k] = ok[k] != 0;
              pp[k] = (uint32_t)pv + pk[k];
              r[k][0] = w0[k] | ((hv[k] >> 8) << 6) | ((hv[k] & 0xffu) << 1);
            }
            bin_put_batch<kHB, 1, true>(B, act, pp, (uint32_t)pv, bins, BS, 1u, r, gp(ps.recs_h), lane, dbg, BST);
          }
        }
      }
    }
  }
}

// Count pass, start of the kernel: the workgroup's partition histogram to zero.
template <int WGS>
__device__ __forceinline__ void pcount_zero(const DevQuery* q, unsigned char* lds_acc) {
  uint32_t* hist = (uint32_t*)lds_acc;
  for (int p = threadIdx.x; p < q->num_parts; p += WGS) hist[p] = 0u;
  __syncthreads();
}

// Count pass, end of the kernel: the histogram to the logical block's row.
template <int WGS>
__device__ __forceinline__ void pcount_store(const DevQuery* q, unsigned char* lds_acc, const PartScratch& ps,
                                             int64_t lb) {
  __syncthreads();
  const uint32_t* hist = (const uint32_t*)lds_acc;
  for (int p = threadIdx.x; p < q->num_parts; p += WGS) gp(ps.hist)[lb * q->num_parts + p] = hist[p];
}

// Emit pass, start of the kernel.
template <int WGS>
__device__ __forceinline__ void pemit_begin(const DevQuery* q, unsigned char* lds_acc, const PartScratch& ps) {
  // every partition's bin empty; its range in the stream: the partition base + this workgroup's offset (part_scan),
  // holding exactly the records the count pass counted here
  const BinState B = bin_state(q, lds_acc);
  const int64_t lbi = q->xcd_major ? xcd_major_block(blockIdx.x, gridDim.x) : (int64_t)blockIdx.x;
  const int P = q->num_parts, pv = q->pv;
  for (int p = q->part_lo + threadIdx.x; p < q->part_hi; p += WGS) {
    B.cnt[p] = 0u;
    B.done[p] = 0u;
    B.front[p] = 0u;
    if (p >= pv) B.slk[p] = 0u;
    B.back[p] = gp(ps.hist)[lbi * P + p];
    B.start[p] = gp(ps.base)[p < pv ? p : p + 1] + gp(ps.off)[lbi * P + p];
  }
  __syncthreads();
}

// Emit pass, end of the kernel (lb: the logical block).
template <int WGS>
__device__ __forceinline__ void pemit_finish(const DevQuery* q, unsigned char* lds_acc, const PartScratch& ps,
                                             int64_t lb) {
  // every bin's rest (< one bin) between the range's front and back, then sentinel records up to the padded end
  __syncthreads();
  const BinState B = bin_state(q, lds_acc);
  const int P = q->num_parts, pv = q->pv;
  for (int p = q->part_lo + threadIdx.x; p < q->part_hi; p += WGS) {
    const bool isv = p < pv;
    const uint32_t nw = isv ? (uint32_t)q->rec_words_v : 1u;
    const uint32_t BS = (uint32_t)(isv ? q->bs_v : q->bs_h);
    const lds_u32_t* bin = isv ? lds_ptr(lds_acc + q->lds_bins_v) + (uint32_t)p * BS * nw
                               : lds_ptr(lds_acc + q->lds_bins_h) + (uint32_t)(p - pv) * (BS + (uint32_t)kDocVals);
    AS1 uint32_t* recs = gp(isv ? ps.recs_v : ps.recs_h);
    const uint32_t n = B.cnt[p], o = B.front[p];
    const uint32_t h = gp(ps.hist)[lb * P + p];
    if ((n >= BS || o + n != B.back[p]) && !q->debug_emit)  // the emit pass must see exactly the count pass's records
      __hip_atomic_fetch_add(gp(q->matched_docs) + 3, 1ull, RLX);
    AS1 uint32_t* d = recs + (B.start[p] + o) * (uint64_t)nw;
    const uint32_t nn = n < BS ? n : BS;
    for (uint32_t e = 0; e < nn * nw; ++e) d[e] = bin[e];
    const uint32_t padded = (h + BS - 1u) / BS * BS;
    AS1 uint32_t* z = recs + (B.start[p] + h) * (uint64_t)nw;
    for (uint32_t e = 0; e < (padded - h) * nw; ++e) z[e] = (e % nw) == 0 ? kSentinel : 0u;
  }
}

}  // namespace pa
