// Scan strategy: FIRSTWITHTIME / LASTWITHTIME, the per-group row picked by time (STRAT_TROW_LDS / STRAT_TROW).
// Included by pa_scan_trow.hip in place of pa_scan.h, which declares the entry points it calls and includes no strategy.
#pragma once
#include "pa_scan.h"

namespace pa {

// ---------------------------------------------------------------- row by time (STRAT_TROW_LDS / STRAT_TROW)
// LASTWITHTIME(v, ts, 'T') / FIRSTWITHTIME(v, ts, 'T'): the reference offers a group's docs in docId order and lets a doc
// whose time is >= (LAST) / <= (FIRST) the best so far take over (LastWithTimeAggregationFunction.java:112,147,196,
// FirstWithTimeAggregationFunction.java:111,147,200), then merges the segments' pairs (:223 / :227). Here the scan keeps,
// per group and time column, the maximum of one synthesized word (TrowDesc, pa_device.h): extreme time first, then the
// greatest (segment bind index, docId) — the reference's rule inside a segment, and this library's rule across the
// segments of a server. Two docs never make the same word, so the result does not depend on the order of the atomics.
// The value column plays no part: pa_query_fetch_time_rows decodes the word and reads any column at the winning row.
//
// The update has the shape of MAX: the lanes of a 64-doc step that share a key reduce their words with wave_max_i64 and
// the leader issues one atomic (ds_max_i64 on the workgroup's LDS copy, or a device-scope 64-bit max); lanes with keys
// of their own issue one each. COUNT and the other aggregations of the query accumulate beside it exactly as in
// accumulate_step (direct key spaces, single-value columns only: the planner refuses the rest).
//
// Wide form (a raw time column whose range does not fit beside the row in 63 bits): the scan is launched twice
// (DevQuery::trow_pass). Launch 1 keeps the maximum of the order-preserving time (complemented for FIRST) in a word of
// its own, next to everything else the query computes; launch 2 walks the same docs (same filter, same admitted keys)
// and a doc whose time equals its key's result takes the maximum of row + 1 into the row word. Launch 2 accumulates
// nothing else: no COUNT, no other aggregation, no numDocsScanned.

typedef __attribute__((address_space(3))) int64_t lds_i64_t;

// x of TrowDesc: the doc's time as the raw INT / LONG value, or the table-wide value id of a dictionary time column
// (DevSeg::hll_lut[a]: the segment's dictId -> table-wide id, nullptr = identity).
__device__ __forceinline__ int64_t trow_time(const DevAgg& A, int a, const DevSeg* __restrict__ seg, const uint32_t* img,
                                             int doc_local, int64_t doc) {
  const DevCol& c = seg->cols[A.slot];
  if (c.kind == COL_SV_DICT) {
    const uint32_t id = decode_dict_id(c, img, doc_local, doc);
    return seg->hll_lut[a] != nullptr ? (int64_t)gp(seg->hll_lut[a])[id] : (int64_t)id;
  }
  return c.vtype == PA_INT ? (int64_t)gp((const int32_t*)c.raw)[doc] : gp((const int64_t*)c.raw)[doc];
}

// max of v into word `key` of the aggregation's accumulator: the workgroup's LDS copy, or `g` in HBM
template <int STRAT>
__device__ __forceinline__ void trow_max(const DevAgg& A, const Acc<STRAT>& acc, int64_t* g, int64_t key, int64_t v) {
  if constexpr (acc_in_lds(STRAT)) __hip_atomic_fetch_max((lds_i64_t*)lds_ptr(acc.lds + A.lds_off) + key, v, WG_RLX);
  else __hip_atomic_fetch_max(gp(g) + key, v, RLX);
}

// One row-by-time aggregation's update for one set of lanes of a 64-doc step (agg_apply_set's contract).
template <int STRAT>
__device__ __forceinline__ void trow_update(const DevAgg& A, const TrowAgg& T, int a, int pass,
                                            const DevSeg* __restrict__ seg, const uint32_t* img, int doc_local,
                                            int64_t doc, int64_t key, int64_t k0, bool in, bool grouped, int leader,
                                            int lane, const Acc<STRAT>& acc) {
  const int64_t x = in ? trow_time(A, a, seg, img, doc_local, doc) : 0;
  const uint64_t row1 = (((uint64_t)(uint32_t)seg->index << T.doc_bits) | (uint64_t)doc) + 1ull;
  int64_t v, idle;
  int64_t* g = A.acc_i64;
  if (!T.wide) {
    v = (int64_t)((((uint64_t)(x - T.tmin) ^ T.flip) << T.row_bits) | row1);
    idle = 0;
  } else if (pass != 2) {
    v = x ^ (int64_t)T.flip;
    idle = INT64_MIN;
    g = T.time;
  } else {
    // (launch 1 has completed: the key's greatest time is final)
    const bool win = in && (x ^ (int64_t)T.flip) == gp(T.time)[key];
    v = win ? (int64_t)row1 : 0;
    idle = 0;
  }
  if (grouped) {
    const int64_t r = wave_max_i64(in ? v : idle);
    if (lane == leader && r != idle) trow_max<STRAT>(A, acc, g, k0, r);
  } else if (in && v != idle) {
    trow_max<STRAT>(A, acc, g, key, v);
  }
}

// Accumulate the matched lanes (`matched` = wave mask) of one 64-doc step: accumulate_step over a direct key space of
// single-value dictionary group-by columns, with the row-by-time aggregations' words beside the ordinary updates.
template <int STRAT>
__device__ __forceinline__ void trow_step(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                          const uint32_t* img, int doc_local, int64_t doc, uint64_t matched, int lane,
                                          const Acc<STRAT>& acc) {
  const TrowDesc* __restrict__ TD = uniform_ptr(q->trow);
  const int pass = q->trow_pass;
  const bool mine = (matched >> lane) & 1ull;
  int64_t key = 0;
  if (mine) {
    for (int j = 0; j < q->num_gb; ++j)
      key += (int64_t)(gb_component(seg->cols[q->gb_slot[j]], seg->remap[j], img, doc_local, doc) *
                       (uint64_t)q->gb_stride[j]);
  }
  uint64_t pending = matched;
  bool first = true;
  while (pending) {
    // (the equal-key sets of accumulate_step)
    const int leader = __builtin_ctzll(pending);
    const int64_t k0 = __shfl(key, leader);
    const uint64_t same = __ballot(key == k0) & pending;
    const bool grouped = !first || (__builtin_popcountll(same) * 4 >= __builtin_popcountll(pending));
    first = false;
    const uint64_t set = grouped ? same : pending;
    pending &= ~set;
    const bool in = (set >> lane) & 1ull;

    if (pass != 2) {
      if (grouped) {
        if (lane == leader) acc.add_count(k0, (uint32_t)__builtin_popcountll(set));
      } else if (in) {
        acc.add_count(key, 1u);
      }
    }
    for (int a = 0; a < q->num_aggs; ++a) {
      const DevAgg& A = q->aggs[a];
      if (A.type == PA_AGG_COUNT) continue;
      if (is_trow_agg(A.type)) {
        const TrowAgg& T = TD->agg[a];
        if (pass == 2 && !T.wide) continue;  // (a packed word is complete after launch 1)
        trow_update<STRAT>(A, T, a, pass, seg, img, doc_local, doc, key, k0, in, grouped, leader, lane, acc);
      } else if (pass != 2) {
        agg_update_set<STRAT>(A, a, seg, img, doc_local, doc, key, k0, in, grouped, leader, lane, acc);
      }
    }
  }
}

// STRAT_TROW_LDS, start of the kernel: the workgroup's LDS accumulators to their identities (lds_acc_zero gives a
// row-by-time word 0; a wide aggregation's word is its time in launch 1: INT64_MIN).
template <int WGS>
__device__ __forceinline__ void trow_lds_zero(const DevQuery* q, unsigned char* lds_acc) {
  lds_acc_zero<WGS>(q, lds_acc);
  if (q->trow_pass != 1) return;
  const int64_t K = q->num_keys;
  for (int a = 0; a < q->num_aggs; ++a) {
    const DevAgg& A = q->aggs[a];
    if (!is_trow_agg(A.type) || !q->trow->agg[a].wide) continue;
    int64_t* r = (int64_t*)(lds_acc + A.lds_off);
    for (int64_t k = threadIdx.x; k < K; k += WGS) r[k] = INT64_MIN;
  }
  __syncthreads();
}

// STRAT_TROW_LDS, end of the kernel: every key the workgroup saw into the global accumulators (lds_acc_flush: counts and
// the ordinary aggregations; not in launch 2, which accumulated none), then the row-by-time words that left their
// identity.
template <int WGS>
__device__ __forceinline__ void trow_lds_flush(const DevQuery* q, unsigned char* lds_acc) {
  const int pass = q->trow_pass;
  if (pass != 2) lds_acc_flush<WGS>(q, lds_acc);
  else __syncthreads();
  const int64_t K = q->num_keys;
  for (int a = 0; a < q->num_aggs; ++a) {
    const DevAgg& A = q->aggs[a];
    if (!is_trow_agg(A.type)) continue;
    const TrowAgg& T = q->trow->agg[a];
    if (pass == 2 && !T.wide) continue;
    const bool time_word = T.wide && pass != 2;
    const int64_t idle = time_word ? INT64_MIN : 0;
    int64_t* g = time_word ? T.time : A.acc_i64;
    const int64_t* r = (const int64_t*)(lds_acc + A.lds_off);
    for (int64_t k = threadIdx.x; k < K; k += WGS) {
      const int64_t w = r[k];
      if (w != idle) __hip_atomic_fetch_max(gp(g) + k, w, RLX);
    }
  }
}

}  // namespace pa
