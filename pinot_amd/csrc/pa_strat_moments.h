// Scan strategy: VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP / COVAR_POP / COVAR_SAMP, the per-group moment sums
// (STRAT_MOM_LDS / STRAT_MOM).
// Included by pa_scan_moments.hip in place of pa_scan.h, which declares the entry points it calls and includes no strategy.
#pragma once
#include "pa_scan.h"

namespace pa {

// ---------------------------------------------------------------- moments (STRAT_MOM_LDS / STRAT_MOM)
// The reference's VarianceAggregationFunction carries (count, sum, m2) per group and updates m2 per doc
// (VarianceTuple.apply); its CovarianceAggregationFunction carries the raw sums of x, y and x y
// (CovarianceAggregationFunction.java:100-108). Here the scan keeps, per group and PA_AGG_MOMENTS aggregation,
// PA_MOMENTS_WORDS = 4 64-bit words that are only ever added to (pinot_amd.h PA_ACC_MOM_I64 / PA_ACC_MOM_F64), and
// pa_query_fetch_moments (pa_moments.hip) finishes the tuple from them and the group's count:
//   integer form  w0 = sum x, w1 = sum y (covariance), w2 / w3 = the low-32 / high-32 sums of p = x * x (variance) or
//                 x * y (covariance). Every argument value lies inside int32, so |p| <= 2^62 and the words are exact for the
//                 2^32 docs a group can hold: integer additions commute, the result does not depend on the order of the
//                 atomics.
//   double form   w0 = sum x', w1 = sum y (covariance), w2 = sum x' * y' in double; variance: x' = y' = x - pivot (m2 is
//                 shift-invariant; the pivot bounds the cancellation of S2 - S1^2 / n by the column's range instead of its
//                 mean), covariance: the reference's own raw sums.
//
// The update has the shape of SUM: the lanes of a 64-doc step that share a key reduce every term across the wave and the
// leader issues one atomic per word (ds_add_u64 / ds_add_f64 on the workgroup's LDS copy, or a device-scope add); lanes
// with keys of their own issue one each. Words that would add zero are skipped (the high word of small squares, w1 of a
// variance). COUNT and the other aggregations of the query accumulate beside it exactly as in accumulate_step (direct key
// spaces, single-value columns only: the planner refuses the rest).

typedef __attribute__((address_space(3))) double lds_f64_t;

struct MomVal {
  int64_t i;  // INT / LONG columns: the value
  double d;   // every column: the value as the reference's getDoubleValuesSV gives it
};

// One argument column's value at a doc: a dictionary column's value through its dictionary, a raw column's as stored.
__device__ __forceinline__ MomVal mom_read(const DevCol& c, const uint32_t* img, int doc_local, int64_t doc) {
  MomVal v{0, 0.0};
  if (c.kind == COL_SV_DICT) {
    const uint32_t id = decode_dict_id(c, img, doc_local, doc);
    if (c.vtype == PA_INT || c.vtype == PA_LONG) {
      v.i = gp(c.dict_i64)[id];
      v.d = (double)v.i;
    } else {
      v.d = gp(c.dict_f64)[id];
    }
  } else {
    switch (c.vtype) {
      case PA_INT: v.i = gp((const int32_t*)c.raw)[doc]; v.d = (double)v.i; break;
      case PA_LONG: v.i = gp((const int64_t*)c.raw)[doc]; v.d = (double)v.i; break;
      case PA_FLOAT: v.d = gp((const float*)c.raw)[doc]; break;
      default: v.d = gp((const double*)c.raw)[doc]; break;
    }
  }
  return v;
}

// v into 64-bit word w of the aggregation's accumulator: the workgroup's LDS copy, or the block in HBM
template <int STRAT>
__device__ __forceinline__ void mom_add_i64(const DevAgg& A, const Acc<STRAT>& acc, int64_t w, int64_t v) {
  if constexpr (acc_in_lds(STRAT)) __hip_atomic_fetch_add((lds_u64_t*)lds_ptr(acc.lds + A.lds_off) + w, (uint64_t)v, WG_RLX);
  else __hip_atomic_fetch_add(gp((unsigned long long*)A.acc_i64) + w, (unsigned long long)v, RLX);
}
template <int STRAT>
__device__ __forceinline__ void mom_add_f64(const DevAgg& A, const Acc<STRAT>& acc, int64_t w, double v) {
  if constexpr (acc_in_lds(STRAT)) __hip_atomic_fetch_add((lds_f64_t*)lds_ptr(acc.lds + A.lds_off) + w, v, WG_RLX);
  else __hip_atomic_fetch_add(gp(A.acc_f64) + w, v, RLX);
}

// One term of one set of lanes (agg_apply_set's contract): reduced across the wave when the set shares key k0.
template <int STRAT>
__device__ __forceinline__ void mom_term_i64(const DevAgg& A, const Acc<STRAT>& acc, int w, int64_t t, int64_t key,
                                             int64_t k0, bool in, bool grouped, int leader, int lane) {
  if (grouped) {
    const int64_t s = wave_sum_i64(in ? t : 0);
    if (lane == leader && s != 0) mom_add_i64<STRAT>(A, acc, PA_MOMENTS_WORDS * k0 + w, s);
  } else if (in && t != 0) {
    mom_add_i64<STRAT>(A, acc, PA_MOMENTS_WORDS * key + w, t);
  }
}
template <int STRAT>
__device__ __forceinline__ void mom_term_f64(const DevAgg& A, const Acc<STRAT>& acc, int w, double t, int64_t key,
                                             int64_t k0, bool in, bool grouped, int leader, int lane) {
  // (t != 0.0 holds for NaN: a NaN reaches its group)
  if (grouped) {
    const double s = wave_sum_f64(in ? t : 0.0);
    if (lane == leader && s != 0.0) mom_add_f64<STRAT>(A, acc, PA_MOMENTS_WORDS * k0 + w, s);
  } else if (in && t != 0.0) {
    mom_add_f64<STRAT>(A, acc, PA_MOMENTS_WORDS * key + w, t);
  }
}

// One PA_AGG_MOMENTS aggregation's update for one set of lanes of a 64-doc step.
template <int STRAT>
__device__ __forceinline__ void mom_update(const DevAgg& A, const MomAgg& M, const DevSeg* __restrict__ seg,
                                           const uint32_t* img, int doc_local, int64_t doc, int64_t key, int64_t k0,
                                           bool in, bool grouped, int leader, int lane, const Acc<STRAT>& acc) {
  const bool cov = M.slot2 >= 0;  // (wave-uniform, like the form: the wave reductions below run in uniform control flow)
  MomVal x{0, 0.0}, y{0, 0.0};
  if (in) {
    x = mom_read(seg->cols[A.slot], img, doc_local, doc);
    if (cov) y = mom_read(seg->cols[M.slot2], img, doc_local, doc);
  }
  if (M.form == PA_MOMENTS_FORM_INTEGER) {
    const int64_t p = x.i * (cov ? y.i : x.i);  // |p| <= 2^62
    mom_term_i64<STRAT>(A, acc, 0, x.i, key, k0, in, grouped, leader, lane);
    if (cov) mom_term_i64<STRAT>(A, acc, 1, y.i, key, k0, in, grouped, leader, lane);
    mom_term_i64<STRAT>(A, acc, 2, (int64_t)(uint32_t)p, key, k0, in, grouped, leader, lane);
    mom_term_i64<STRAT>(A, acc, 3, p >> 32, key, k0, in, grouped, leader, lane);
  } else {
    const double dx = cov ? x.d : x.d - M.pivot;
    const double dy = cov ? y.d : dx;
    mom_term_f64<STRAT>(A, acc, 0, dx, key, k0, in, grouped, leader, lane);
    if (cov) mom_term_f64<STRAT>(A, acc, 1, dy, key, k0, in, grouped, leader, lane);
    mom_term_f64<STRAT>(A, acc, 2, dx * dy, key, k0, in, grouped, leader, lane);
  }
}

// Accumulate the matched lanes (`matched` = wave mask) of one 64-doc step: accumulate_step over a direct key space of
// single-value dictionary group-by columns, with the moment sums beside the ordinary updates.
template <int STRAT>
__device__ __forceinline__ void mom_step(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                         const uint32_t* img, int doc_local, int64_t doc, uint64_t matched, int lane,
                                         const Acc<STRAT>& acc) {
  const MomDesc* __restrict__ MD = uniform_ptr(q->mom);
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

    if (grouped) {
      if (lane == leader) acc.add_count(k0, (uint32_t)__builtin_popcountll(set));
    } else if (in) {
      acc.add_count(key, 1u);
    }
    for (int a = 0; a < q->num_aggs; ++a) {
      const DevAgg& A = q->aggs[a];
      if (A.type == PA_AGG_COUNT) continue;
      if (A.type == PA_AGG_MOMENTS)
        mom_update<STRAT>(A, MD->agg[a], seg, img, doc_local, doc, key, k0, in, grouped, leader, lane, acc);
      else
        agg_update_set<STRAT>(A, a, seg, img, doc_local, doc, key, k0, in, grouped, leader, lane, acc);
    }
  }
}

// STRAT_MOM_LDS, start of the kernel: the workgroup's LDS accumulators to their identities (lds_acc_zero clears the
// first K words of a PA_AGG_MOMENTS block; the block is PA_MOMENTS_WORDS * K words, all zero: 0.0 is all-zero bits).
template <int WGS>
__device__ __forceinline__ void mom_lds_zero(const DevQuery* q, unsigned char* lds_acc) {
  lds_acc_zero<WGS>(q, lds_acc);
  const int64_t n = q->num_keys * PA_MOMENTS_WORDS;
  for (int a = 0; a < q->num_aggs; ++a) {
    const DevAgg& A = q->aggs[a];
    if (A.type != PA_AGG_MOMENTS) continue;
    uint64_t* r = (uint64_t*)(lds_acc + A.lds_off);
    for (int64_t k = threadIdx.x; k < n; k += WGS) r[k] = 0;
  }
  __syncthreads();
}

// STRAT_MOM_LDS, end of the kernel: every key the workgroup saw into the global accumulators (lds_acc_flush: counts and
// the ordinary aggregations; it leaves a PA_AGG_MOMENTS block alone), then every non-zero moment word as one global add.
template <int WGS>
__device__ __forceinline__ void mom_lds_flush(const DevQuery* q, unsigned char* lds_acc) {
  lds_acc_flush<WGS>(q, lds_acc);
  const int64_t n = q->num_keys * PA_MOMENTS_WORDS;
  for (int a = 0; a < q->num_aggs; ++a) {
    const DevAgg& A = q->aggs[a];
    if (A.type != PA_AGG_MOMENTS) continue;
    const uint64_t* r = (const uint64_t*)(lds_acc + A.lds_off);
    if (q->mom->agg[a].form == PA_MOMENTS_FORM_INTEGER) {
      for (int64_t k = threadIdx.x; k < n; k += WGS) {
        const uint64_t w = r[k];
        if (w != 0) __hip_atomic_fetch_add(gp((unsigned long long*)A.acc_i64) + k, (unsigned long long)w, RLX);
      }
    } else {
      for (int64_t k = threadIdx.x; k < n; k += WGS) {
        const uint64_t w = r[k];  // (the bits: -0.0 and NaN are non-zero words; adding -0.0 changes nothing)
        if (w != 0) __hip_atomic_fetch_add(gp(A.acc_f64) + k, __builtin_bit_cast(double, w), RLX);
      }
    }
  }
}

}  // namespace pa
