// Distinct queries (include/pinot_amd.h "distinct queries"): what follows the scan's key-presence bitmap
// (pa_strat_distinct.h "distinct"), and their host side.
//
// Finish. The rows are the first min(limit, P) present keys under the completed order (DstOrder). When that order is
// the raw key's own digit order, the rows are the first set bits of the scan's bitmap: per block of bitmap words a
// popcount, block prefixes by scan_u64_kernel, then every block below the limit ranks its bits and writes their
// component ids. Otherwise every present key is first re-keyed: its sort key (a bijection of the key, below num_keys)
// sets one bit of a second bitmap of the same size, and the same rank pass over that bitmap gives the rows in final
// order: ordering P present keys costs one pass over the key space's bits, whatever the limit.
#include "pa_host.h"
#include "pa_strat_distinct.h"

namespace pa {

constexpr int kDstThreads = 256;
constexpr int kDstWordsPerThread = 16;
constexpr int64_t kDstBlockWords = (int64_t)kDstThreads * kDstWordsPerThread;  // 131072 keys per block

// counts[b] = set bits of block b's words
__global__ void __launch_bounds__(kDstThreads) dst_count_kernel(const uint32_t* __restrict__ bits, int64_t words,
                                                                 uint64_t* __restrict__ counts) {
  __shared__ uint32_t sh[kDstThreads / kWave];
  const int64_t w0 = (int64_t)blockIdx.x * kDstBlockWords + (int64_t)threadIdx.x * kDstWordsPerThread;
  uint32_t c = 0;
#pragma unroll
  for (int k = 0; k < kDstWordsPerThread; ++k)
    if (w0 + k < words) c += (uint32_t)__builtin_popcount(bits[w0 + k]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < kDstThreads / kWave; ++w) t += sh[w];
    counts[blockIdx.x] = t;
  }
}

// every present key's sort key into the second bitmap (zeroed before)
__global__ void __launch_bounds__(kDstThreads) dst_rekey_kernel(const uint32_t* __restrict__ bits, int64_t words,
                                                                 uint32_t* __restrict__ bits2, DstOrder o) {
  for (int64_t w = (int64_t)blockIdx.x * kDstThreads + threadIdx.x; w < words; w += (int64_t)gridDim.x * kDstThreads) {
    uint32_t v = bits[w];
    while (v) {
      const int b = __builtin_ctz(v);
      v &= v - 1;
      uint32_t key = (uint32_t)w * 32u + (uint32_t)b;
      uint32_t id[PA_MAX_GROUP_BY];
      for (int j = 0; j < o.n; ++j) {  // the raw key's digits: column 0 least significant
        const uint32_t c = (uint32_t)o.kcard[j];
        id[j] = key % c;
        key /= c;
      }
      uint32_t sk = 0;
      for (int i = o.n - 1; i >= 0; --i) {
        const uint32_t c = (uint32_t)o.card[i];
        const uint32_t d = o.desc[i] ? c - 1u - id[o.col[i]] : id[o.col[i]];
        sk = sk * c + d;
      }
      __hip_atomic_fetch_or(gp(bits2) + (sk >> 5), 1u << (sk & 31u), RLX);
    }
  }
}

// rows [0, limit) in rank order: base[b] = set bits before block b (the scanned counts); row r = the component ids of
// the r-th set bit, decoded digit by digit (o: least significant first)
__global__ void __launch_bounds__(kDstThreads) dst_emit_kernel(const uint32_t* __restrict__ bits, int64_t words,
                                                                const uint64_t* __restrict__ base, uint64_t limit,
                                                                int32_t* __restrict__ rows, DstOrder o) {
  __shared__ uint32_t sh[kDstThreads / kWave];
  const uint64_t b0 = base[blockIdx.x];
  if (b0 >= limit) return;  // (block-uniform: blocks past the limit do nothing)
  const int64_t w0 = (int64_t)blockIdx.x * kDstBlockWords + (int64_t)threadIdx.x * kDstWordsPerThread;
  uint32_t wv[kDstWordsPerThread];
  uint32_t c = 0;
#pragma unroll
  for (int k = 0; k < kDstWordsPerThread; ++k) {
    wv[k] = w0 + k < words ? bits[w0 + k] : 0u;
    c += (uint32_t)__builtin_popcount(wv[k]);
  }
  // exclusive prefix of c over the block's threads
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = c;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)incl, d, kWave);
    if (lane >= d) incl += t;
  }
  if (lane == kWave - 1) sh[wave] = incl;
  __syncthreads();
  uint32_t before = 0;
  for (int w = 0; w < wave; ++w) before += sh[w];
  uint64_t r = b0 + before + (incl - c);
#pragma unroll
  for (int k = 0; k < kDstWordsPerThread; ++k) {
    uint32_t v = wv[k];
    while (v && r < limit) {
      const int b = __builtin_ctz(v);
      v &= v - 1;
      uint32_t sk = (uint32_t)(w0 + k) * 32u + (uint32_t)b;
      for (int i = 0; i < o.n; ++i) {
        const uint32_t cd = (uint32_t)o.card[i];
        const uint32_t d = sk % cd;
        sk /= cd;
        rows[r * (uint64_t)o.n + (uint64_t)o.col[i]] = (int32_t)(o.desc[i] ? cd - 1u - d : d);
      }
      ++r;
    }
  }
}

}  // namespace pa

// ---------------------------------------------------------------- prepare
// The DISTINCT columns against the bound segments, the direct key space with its own bound, and the completed order.
int distinct_key_space(pa_query* q, Prep& P) {
  const pa_query_spec& s = q->spec;
  const pa_distinct_spec& ds = q->dst_spec;
  q->hashed = false;
  q->key_words = 1;
  P.gb_word.assign(s.num_group_by, 0);
  P.gb_raw.assign(s.num_group_by, 0);
  P.stride.assign(s.num_group_by, 0);
  if (s.num_group_by < 1) return fail(PA_EINVAL, "distinct: no columns");
  if (s.num_aggs != 0) return fail(PA_EINVAL, "distinct: the spec must have no aggregations");
  int64_t K = 1;
  for (int j = 0; j < s.num_group_by; ++j) {
    for (int si = 0; si < q->nseg; ++si) {
      auto it = q->segs[si]->cols.find(s.group_by_columns[j]);
      if (it == q->segs[si]->cols.end())
        return fail(PA_EINVAL, "distinct: column " + std::to_string(s.group_by_columns[j]) + " missing in a segment");
      const Column* c = it->second;
      if (c->kind == COL_SV_RAW)
        return fail(PA_EUNSUPPORTED, "distinct: raw (no-dictionary) column " + std::to_string(s.group_by_columns[j]) +
                                     " is not supported");
      if (c->kind == COL_MV_DICT)
        return fail(PA_EUNSUPPORTED, "distinct: multi-value column " + std::to_string(s.group_by_columns[j]) +
                                     " is not supported");
      if (c->vtype == PA_BYTES)
        return fail(PA_EUNSUPPORTED, "distinct: BYTES column " + std::to_string(s.group_by_columns[j]) +
                                     " is not supported");
    }
    const int64_t card = s.group_by_cardinality[j];
    if (card < 1) return fail(PA_EINVAL, "group_by_cardinality < 1 for a dictionary column");
    P.stride[j] = K;
    if (card > kDistinctMaxKeys || K > kDistinctMaxKeys / card)
      return fail(PA_EUNSUPPORTED, "distinct: the key space (product of the column cardinalities) exceeds 2^31 keys; "
                                   "a hashed key set is not supported");
    K *= card;
  }
  q->num_keys = K;
  if (ds.num_order_by > 0 && ds.limit > PA_MAX_SELECT_ROWS && K > PA_MAX_SELECT_ROWS)
    return fail(PA_EUNSUPPORTED, "distinct: ORDER BY with limit " + std::to_string(ds.limit) +
                                 " exceeds PA_MAX_SELECT_ROWS (" + std::to_string(PA_MAX_SELECT_ROWS) + ")");
  // completed order, most significant first: the ORDER BY entries, then the columns they do not name, ascending, in
  // select order; DstOrder keeps it least significant first
  const int n = s.num_group_by;
  std::vector<int> col, desc;
  std::vector<char> named(n, 0);
  for (int i = 0; i < ds.num_order_by; ++i) {
    col.push_back(ds.order_by_index[i]);
    desc.push_back(ds.order_by_desc[i] ? 1 : 0);
    named[ds.order_by_index[i]] = 1;
  }
  for (int j = 0; j < n; ++j)
    if (!named[j]) {
      col.push_back(j);
      desc.push_back(0);
    }
  DstOrder& o = q->dst_order;
  std::memset(&o, 0, sizeof(o));
  o.n = n;
  q->dst_key_order = true;  // the raw key's digit order: column i is digit i, ascending
  for (int i = 0; i < n; ++i) {
    o.col[i] = col[n - 1 - i];
    o.desc[i] = desc[n - 1 - i];
    o.card[i] = (int32_t)std::min<int64_t>(s.group_by_cardinality[o.col[i]], INT32_MAX);
    o.kcard[i] = (int32_t)std::min<int64_t>(s.group_by_cardinality[i], INT32_MAX);
    if (o.col[i] != i || o.desc[i]) q->dst_key_order = false;
  }
  return PA_OK;
}

int distinct_plan(pa_query* q) {
  const int64_t words = (q->num_keys + 31) / 32;
  const int64_t nb = (words + kDstBlockWords - 1) / kDstBlockWords;
  if (int rc = dev_alloc(q->dst_counts, (size_t)(nb + 1) * 8)) return rc;
  if (!q->dst_key_order)
    if (int rc = dev_alloc(q->dst_bits2, (size_t)words * 4)) return rc;
  return PA_OK;
}

// ---------------------------------------------------------------- C-ABI
extern "C" {

int pa_query_set_distinct(pa_query* q, const pa_distinct_spec* spec) {
  if (!q || !spec) return fail(PA_EINVAL, "bad distinct arguments");
  if (q->prepared) return fail(PA_EINVAL, "query already prepared");
  if (q->is_select) return fail(PA_EINVAL, "a selection cannot be distinct");
  const int n = q->spec.num_group_by;
  if (n < 1 || q->spec.num_aggs != 0)
    return fail(PA_EINVAL, "a distinct query is made from a GROUP BY spec without aggregations");
  if (spec->num_order_by < 0 || spec->num_order_by > n) return fail(PA_EINVAL, "distinct: num_order_by out of range");
  if (spec->limit < 0) return fail(PA_EINVAL, "distinct: negative limit");
  std::vector<char> seen(n, 0);
  for (int i = 0; i < spec->num_order_by; ++i) {
    const int j = spec->order_by_index[i];
    if (j < 0 || j >= n || seen[j]) return fail(PA_EINVAL, "distinct: ORDER BY entries index each DISTINCT column at most once");
    seen[j] = 1;
  }
  q->is_distinct = true;
  q->dst_spec = *spec;
  q->spec.num_groups_limit = 0;
  return PA_OK;
}

int64_t pa_query_fetch_distinct(pa_query* q, void* stream, int64_t capacity, int32_t* out_ids, int64_t* out_present) {
  if (!q || !q->prepared) return fail(PA_EINVAL, "query not prepared");
  if (!q->is_distinct) return fail(PA_EINVAL, "not a distinct query");
  if (capacity < 0) return fail(PA_EINVAL, "negative capacity");
  if (const char* t = tuning_invalidating(q->tune))
    return fail(PA_EINVAL, std::string("results invalid: tuning ") + t + " is set");
  hipStream_t st = (hipStream_t)stream;
  const int64_t words = (q->num_keys + 31) / 32;
  const int64_t nb = (words + kDstBlockWords - 1) / kDstBlockWords;
  const uint32_t* bits = (const uint32_t*)q->sections[0].ptr;
  const DstOrder& o = q->dst_order;
  DstOrder ko = o;  // the raw key's own digits
  for (int i = 0; i < o.n; ++i) {
    ko.col[i] = i;
    ko.desc[i] = 0;
    ko.card[i] = o.kcard[i];
  }
  if (!q->dst_key_order) {
    PA_HIP(hipMemsetAsync(q->dst_bits2.p, 0, (size_t)words * 4, st));
    const unsigned grid = (unsigned)std::min<int64_t>(4096, (words + kDstThreads - 1) / kDstThreads);
    hipLaunchKernelGGL(dst_rekey_kernel, dim3(grid), dim3(kDstThreads), 0, st, bits, words, (uint32_t*)q->dst_bits2.p, o);
    PA_HIP(hipGetLastError());
    bits = (const uint32_t*)q->dst_bits2.p;
  }
  uint64_t* counts = (uint64_t*)q->dst_counts.p;
  hipLaunchKernelGGL(dst_count_kernel, dim3((unsigned)nb), dim3(kDstThreads), 0, st, bits, words, counts);
  PA_HIP(hipGetLastError());
  PA_HIP(launch_scan_u64(counts, nb, st));
  uint64_t present = 0, md[4] = {0, 0, 0, 0};
  PA_HIP(hipMemcpyAsync(&present, counts + nb, 8, hipMemcpyDeviceToHost, st));
  PA_HIP(hipMemcpyAsync(md, q->sections.back().ptr, 32, hipMemcpyDeviceToHost, st));
  PA_HIP(hipStreamSynchronize(st));
  q->last_matched = (int64_t)md[0];
  q->scanned_since_fetch = false;
  if (out_present) *out_present = (int64_t)present;
  const int64_t R = std::min<int64_t>((int64_t)present, q->dst_spec.limit);
  const int64_t n = std::min(R, capacity);
  if (n > 0 && out_ids) {
    const size_t bytes = (size_t)n * o.n * 4;
    if (q->dst_rows.n < bytes) {
      dev_free(q->dst_rows);
      if (int rc = dev_alloc(q->dst_rows, bytes)) return rc;
    }
    hipLaunchKernelGGL(dst_emit_kernel, dim3((unsigned)nb), dim3(kDstThreads), 0, st, bits, words, counts, (uint64_t)n,
                       (int32_t*)q->dst_rows.p, q->dst_key_order ? ko : o);
    PA_HIP(hipGetLastError());
    PA_HIP(hipMemcpyAsync(out_ids, q->dst_rows.p, bytes, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
  }
  return R;
}

}  // extern "C"
