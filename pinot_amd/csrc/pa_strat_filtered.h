// Scan strategy: filtered aggregations (STRAT_FILTERED_LDS / STRAT_FILTERED).
// Included by pa_scan_filtered.hip in place of pa_scan.h, which declares the entry points it calls and includes no strategy.
#pragma once
#include "pa_scan.h"

namespace pa {

// ---------------------------------------------------------------- filtered aggregations (STRAT_FILTERED_LDS / STRAT_FILTERED)
// AGG(x) FILTER (WHERE F_j): the reference runs one filter + projection + executor per "swim lane"
// (FilteredAggregationOperator.java:66-101, FilteredGroupByOperator.java:107-200: a walk over the segment per lane).
// Here the columns stream once: after the query's own filter W left the tile's survivors m, every lane's CNF (FiltDesc)
// gives m_j = m & F_j — literals on staged dictionary columns on the whole tile (leaf_bits), the others per surviving
// doc (leaf_match_doc) — and the group key is computed once per doc of the lanes' union u (the shared group-key
// generator, FilteredGroupByOperator.java:117-150: a group exists when any lane saw a doc of it; the group count
// counts u). Lane j then accumulates its aggregations and its doc count (PA_ACC_LANE_COUNT_U64) under its own mask
// with accumulate_step's wave pre-reduction; aggregations without a filter run under m (the main lane). Per segment
// the docs of W and of every lane are counted by popcount (the execution statistics' input).
//   STRAT_FILTERED_LDS: group counts, lane counts and every aggregation workgroup-private in LDS (the STRAT_LDS layout
//     + u32 lane counts), flushed once per workgroup: one global atomic per cell of a lane that saw the key.
//   STRAT_FILTERED: device-scope atomics per pre-reduced set.
// Direct key spaces and single-value columns only (pa_query_prepare refuses the rest), step-major tiles.

// Lane mask of one CNF (n literals, clause-major) over the tile's surviving docs m.
template <int STEPS>
__device__ __forceinline__ uint32_t filt_lane_mask(const DevLeaf* lits, int n, const uint32_t* img, int64_t doc_base,
                                                   uint32_t m, int lane) {
  uint32_t mj = m, clause = 0;
  for (int li = 0; li < n; ++li) {
    const DevLeaf& L = lits[li];
    uint32_t bits = 0;
    if ((L.kind == PA_LEAF_DICT_RANGE || L.kind == PA_LEAF_DICT_SET) && L.lds_off >= 0) {
      bits = leaf_bits<STEPS>(L, img, doc_base, lane);
    } else {
      // not staged (or a raw column): only docs that can still change the lane's mask, each a doc of the segment
      const uint32_t todo = mj & ~clause;
      for (int i = 0; i < STEPS; ++i) {
        if (__ballot((todo >> i) & 1u) == 0) continue;
        if ((todo >> i) & 1u) bits |= (uint32_t)leaf_match_doc(L, doc_base + i * kWave + lane) << i;
      }
    }
    clause |= bits;
    if (L.clause_end) {
      mj &= clause;
      clause = 0;
    }
  }
  return mj & m;  // (a negated leaf sets bits past the segment's last doc: process_tile)
}

// Lane j's mask out of the four pairs filtered_tile keeps (values, not references: a conditional between two lvalues
// selects an address, and the masks would have to live in memory).
__device__ __forceinline__ uint32_t filt_pair_mask(uint64_t p0, uint64_t p1, uint64_t p2, uint64_t p3, int j) {
  const uint64_t k = (uint64_t)(j >> 1);
  const uint64_t p = (p0 & (0ull - (uint64_t)(k == 0))) | (p1 & (0ull - (uint64_t)(k == 1))) |
                     (p2 & (0ull - (uint64_t)(k == 2))) | (p3 & (0ull - (uint64_t)(k == 3)));
  return (uint32_t)(p >> ((j & 1) * 32));
}

// One lane's docs of one 64-doc step (`set_mask`: wave mask) into the lane's doc count and aggregations: the equal-key
// sets of accumulate_step. cell0 < 0: the count is the group's (Acc::add_count), else the lane count at cell0 + key.
template <int STRAT>
__device__ __forceinline__ void filtered_lane_step(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                                   const uint32_t* img, int doc_local, int64_t doc, int64_t key,
                                                   uint64_t set_mask, int lane, const Acc<STRAT>& acc,
                                                   const int32_t* aggs, int naggs, int64_t cell0) {
  uint64_t pending = set_mask;
  bool first = true;
  while (pending) {
    const int leader = __builtin_ctzll(pending);
    const int64_t k0 = __shfl(key, leader);
    const uint64_t same = __ballot(key == k0) & pending;
    const bool grouped = !first || (__builtin_popcountll(same) * 4 >= __builtin_popcountll(pending));
    first = false;
    const uint64_t set = grouped ? same : pending;
    pending &= ~set;
    const bool in = (set >> lane) & 1ull;
    if (grouped) {
      if (lane == leader) {
        if (cell0 < 0) acc.add_count(k0, (uint32_t)__builtin_popcountll(set));
        else acc.add_lane_count(cell0 + k0, (uint32_t)__builtin_popcountll(set));
      }
    } else if (in) {
      if (cell0 < 0) acc.add_count(key, 1u);
      else acc.add_lane_count(cell0 + key, 1u);
    }
    for (int x = 0; x < naggs; ++x) {
      const int a = aggs[x];
      agg_update_set<STRAT>(q->aggs[a], a, seg, img, doc_local, doc, key, k0, in, grouped, leader, lane, acc);
    }
  }
}

// The docs of one tile that passed W (bit i of m: the lane's doc of step i): lane masks, counters, aggregation.
template <int STRAT, int STEPS>
__device__ __forceinline__ void filtered_tile(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                              const uint32_t* img, int64_t doc_base, uint32_t m, int lane,
                                              const Acc<STRAT>& acc) {
  const FiltDesc* __restrict__ F = uniform_ptr(q->filt);
  const int NL = F->num_lanes;
  const bool has_main = F->has_main != 0;
  const DevLeaf* lits = uniform_ptr(F->leaves + (int64_t)seg->index * F->num_lits);
  // the lanes' masks, two to a 64-bit scalar (lane j: bits 32 (j & 1) .. of pair j >> 1). Named scalars, not an array:
  // an array indexed by the lane number stays in scratch memory, whose loads and stores wait behind the DMA ring.
  static_assert(PA_MAX_AGG_FILTERS == 8 && STEPS <= 32, "four pairs of 32-bit lane masks");
  uint64_t p0 = 0, p1 = 0, p2 = 0, p3 = 0;
  uint32_t u = has_main ? m : 0u;
  for (int j = 0; j < NL; ++j) {
    const int b = F->lit_begin[j];
    const uint32_t mj = filt_lane_mask<STEPS>(lits + b, F->lit_begin[j + 1] - b, img, doc_base, m, lane);
    const uint64_t w = (uint64_t)mj << ((j & 1) * 32);
    p0 |= (j >> 1) == 0 ? w : 0ull;
    p1 |= (j >> 1) == 1 ? w : 0ull;
    p2 |= (j >> 1) == 2 ? w : 0ull;
    p3 |= (j >> 1) == 3 ? w : 0ull;
    u |= mj;
  }
  AS1 unsigned long long* sd = gp(F->seg_docs) + (int64_t)seg->index * (NL + 1);
  {
    const int64_t w = wave_sum_i64((int64_t)__builtin_popcount(m));
    if (lane == 0 && w != 0) __hip_atomic_fetch_add(sd, (unsigned long long)w, RLX);
  }
  for (int j = 0; j < NL; ++j) {
    const int64_t c = wave_sum_i64((int64_t)__builtin_popcount(filt_pair_mask(p0, p1, p2, p3, j)));
    if (lane == 0 && c != 0) __hip_atomic_fetch_add(sd + 1 + j, (unsigned long long)c, RLX);
  }
  if (__ballot(u != 0) == 0) return;
  const int64_t K = q->num_keys;
  for (int i = 0; i < STEPS; ++i) {
    const uint64_t um = __ballot((u >> i) & 1u);
    if (um == 0) continue;
    const int doc_local = i * kWave + lane;
    const int64_t doc = doc_base + doc_local;
    int64_t key = 0;
    if ((um >> lane) & 1ull)
      for (int j = 0; j < q->num_gb; ++j)
        key += (int64_t)(gb_component(seg->cols[q->gb_slot[j]], seg->remap[j], img, doc_local, doc) *
                         (uint64_t)q->gb_stride[j]);
    // the group count under the union, with the main lane's aggregations when there is one (then u == m)
    filtered_lane_step<STRAT>(q, seg, img, doc_local, doc, key, um, lane, acc, F->lane_aggs[NL],
                              has_main ? F->lane_naggs[NL] : 0, -1);
    for (int j = 0; j < NL; ++j) {
      const uint64_t jm = __ballot((filt_pair_mask(p0, p1, p2, p3, j) >> i) & 1u);
      if (jm == 0) continue;
      filtered_lane_step<STRAT>(q, seg, img, doc_local, doc, key, jm, lane, acc, F->lane_aggs[j], F->lane_naggs[j],
                                (int64_t)j * K);
    }
  }
}

// STRAT_FILTERED_LDS, start of the kernel: the workgroup's lane counts to zero, then the STRAT_LDS accumulators.
template <int WGS>
__device__ __forceinline__ void filtered_lds_zero(const DevQuery* q, unsigned char* lds_acc) {
  const FiltDesc* F = q->filt;
  uint32_t* lc = (uint32_t*)(lds_acc + F->lds_lane_count_off);
  const int64_t n = (int64_t)F->num_lanes * q->num_keys;
  for (int64_t k = threadIdx.x; k < n; k += WGS) lc[k] = 0u;
  lds_acc_zero<WGS>(q, lds_acc);
}

// STRAT_FILTERED_LDS, end of the kernel: for every key the workgroup saw, the group count, and for every lane that saw
// it the lane count and that lane's aggregations (the cells of the other lanes hold identities: nothing to send).
template <int WGS>
__device__ __forceinline__ void filtered_lds_flush(const DevQuery* q, unsigned char* lds_acc) {
  __syncthreads();
  const FiltDesc* F = q->filt;
  const int64_t K = q->num_keys;
  const int NL = F->num_lanes;
  const uint32_t* cnt = (const uint32_t*)(lds_acc + q->lds_count_off);
  const uint32_t* lc = (const uint32_t*)(lds_acc + F->lds_lane_count_off);
  for (int64_t k = threadIdx.x; k < K; k += WGS) {
    const uint32_t c = cnt[k];
    if (c == 0) continue;
    __hip_atomic_fetch_add(gp(q->count) + k, (unsigned long long)c, RLX);
    for (int j = 0; j <= NL; ++j) {
      if (j < NL) {
        const uint32_t n = lc[(int64_t)j * K + k];
        if (n == 0) continue;
        __hip_atomic_fetch_add(gp(F->lane_count) + (int64_t)j * K + k, (unsigned long long)n, RLX);
      } else if (!F->has_main) {
        break;
      }
      for (int x = 0; x < F->lane_naggs[j]; ++x) lds_flush_agg(q->aggs[F->lane_aggs[j][x]], k, lds_acc);
    }
  }
}

}  // namespace pa
