// VALUE_HISTOGRAM results (PA_ACC_HIST_U64: [key * stride + value id] 64-bit bins): pa_query_fetch_histogram (the
// non-zero bins of every fetched group as (value id, count) pairs) and pa_query_percentiles (a rank select over each
// fetched group's bins). One workgroup (one wave for short rows) per fetched group; a row streams as coalesced 8-byte
// loads, 64 or 256 bins per pass with a running total, so a row of any length (21,910 values, 50,000 values) takes
// stride / threads passes and no host loop ever touches a bin.
#include "pa_host.h"

namespace {

constexpr int kHistWG = 256;        // threads per group for long rows
constexpr int kHistShortRow = 1024;  // rows up to this many bins take one wave per group

// Sum over the workgroup's T threads (T = 64: one wave, no LDS); every thread gets it. sh: T / 64 words.
template <int T>
__device__ __forceinline__ uint64_t block_sum_u64(uint64_t v, uint64_t* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o);
  if (T == 64) return v;
  const int wave = threadIdx.x >> 6;
  __syncthreads();  // (sh may still be read by the previous call)
  if ((threadIdx.x & 63) == 0) sh[wave] = v;
  __syncthreads();
  uint64_t s = 0;
#pragma unroll
  for (int w = 0; w < T / 64; ++w) s += sh[w];
  return s;
}

// Inclusive prefix sum over the workgroup's T threads; *total = the sum of all. sh: T / 64 words.
template <int T>
__device__ __forceinline__ uint64_t block_inclusive_scan_u64(uint64_t v, uint64_t* sh, uint64_t* total) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t y = (uint64_t)__shfl_up((unsigned long long)v, o);
    if (lane >= o) v += y;
  }
  if (T == 64) {
    *total = (uint64_t)__shfl((unsigned long long)v, 63);
    return v;
  }
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 63) sh[wave] = v;
  __syncthreads();
  uint64_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < T / 64; ++w) {
    const uint64_t s = sh[w];
    if (w < wave) before += s;
    all += s;
  }
  *total = all;
  return v + before;
}

// nz[g] = non-zero bins of fetched group g's row
template <int T>
__global__ void __launch_bounds__(T) hist_count_kernel(const uint64_t* __restrict__ hist, int64_t stride,
                                                       const int64_t* __restrict__ keys, uint64_t* __restrict__ nz) {
  __shared__ uint64_t sh[4];
  const uint64_t* row = hist + keys[blockIdx.x] * stride;
  uint64_t c = 0;
  for (int64_t i = threadIdx.x; i < stride; i += T) c += row[i] != 0;
  c = block_sum_u64<T>(c, sh);
  if (threadIdx.x == 0) nz[blockIdx.x] = c;
}

// single workgroup: in-place exclusive scan of n 64-bit counts; v[n] = total
__global__ void __launch_bounds__(kHistWG) hist_scan_kernel(uint64_t* v, int64_t n) {
  __shared__ uint64_t sh[4];
  uint64_t carry = 0;
  for (int64_t b0 = 0; b0 < n; b0 += kHistWG) {
    const int64_t i = b0 + threadIdx.x;
    const uint64_t x = i < n ? v[i] : 0ull;
    uint64_t tot;
    const uint64_t incl = block_inclusive_scan_u64<kHistWG>(x, sh, &tot);
    if (i < n) v[i] = carry + incl - x;
    carry += tot;
  }
  if (threadIdx.x == 0) v[n] = carry;
}

// Group g's non-zero bins, in ascending value id, to pairs [off[g], off[g + 1]) (those below cap): each pass ranks its
// non-zero bins by ballot + popcount, so consecutive pairs are stored by consecutive lanes.
template <int T>
__global__ void __launch_bounds__(T) hist_compact_kernel(const uint64_t* __restrict__ hist, int64_t stride,
                                                         const int64_t* __restrict__ keys,
                                                         const uint64_t* __restrict__ off, int64_t cap,
                                                         int32_t* __restrict__ ids, int64_t* __restrict__ counts) {
  __shared__ uint32_t sh[2][4];  // (two buffers: one barrier per pass)
  const uint64_t* row = hist + keys[blockIdx.x] * stride;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t pos0 = (int64_t)off[blockIdx.x];
  int buf = 0;
  for (int64_t b0 = 0; b0 < stride; b0 += T, buf ^= 1) {
    const int64_t i = b0 + threadIdx.x;
    const uint64_t x = i < stride ? row[i] : 0ull;
    const uint64_t m = __ballot(x != 0);
    uint32_t before = (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
    uint32_t all = (uint32_t)__builtin_popcountll(m);
    if (T > 64) {
      if (lane == 0) sh[buf][wave] = all;
      __syncthreads();
      all = 0;
#pragma unroll
      for (int w = 0; w < T / 64; ++w) {
        const uint32_t s = sh[buf][w];
        if (w < wave) before += s;
        all += s;
      }
    }
    const int64_t p = pos0 + before;
    if (x != 0 && p < cap) {
      ids[p] = (int32_t)i;
      counts[p] = (int64_t)x;
    }
    pos0 += all;
  }
}

// Rank select: out[g * np + j] = the first bin of group g's row whose inclusive prefix sum exceeds the rank of
// pct[j] (PercentileAggregationFunction.extractFinalResult over the sorted values), -1 for an all-zero row. The total
// first (one streaming pass), then the ranks, then a second pass of block prefix sums with a running total in which
// every non-zero bin tests all ranks: all percentiles of the row are located in the same pass.
template <int T>
__global__ void __launch_bounds__(T) hist_select_kernel(const uint64_t* __restrict__ hist, int64_t stride,
                                                        const int64_t* __restrict__ keys, int np,
                                                        const double* __restrict__ pct, int32_t* __restrict__ out) {
  __shared__ uint64_t sh[4];
  __shared__ uint64_t ranks[PA_MAX_PERCENTILES];
  const uint64_t* row = hist + keys[blockIdx.x] * stride;
  int32_t* o = out + (int64_t)blockIdx.x * np;
  uint64_t total = 0;
  for (int64_t i = threadIdx.x; i < stride; i += T) total += row[i];
  total = block_sum_u64<T>(total, sh);
  if (total == 0) {  // (uniform)
    if ((int)threadIdx.x < np) o[threadIdx.x] = -1;
    return;
  }
  if ((int)threadIdx.x < np) {
    const double p = pct[threadIdx.x];
    // values[size - 1] at 100, else values[(int) ((long) size * percentile / 100)] (a rank a rounded product could
    // push to `size` is held at the last value)
    uint64_t r = p == 100.0 ? total - 1 : (uint64_t)(int64_t)((double)total * p / 100.0);
    ranks[threadIdx.x] = r < total ? r : total - 1;
  }
  __syncthreads();
  uint64_t carry = 0;
  for (int64_t b0 = 0; b0 < stride; b0 += T) {
    const int64_t i = b0 + threadIdx.x;
    const uint64_t x = i < stride ? row[i] : 0ull;
    uint64_t tot;
    const uint64_t incl = carry + block_inclusive_scan_u64<T>(x, sh, &tot);
    if (x != 0) {
      const uint64_t excl = incl - x;
      for (int j = 0; j < np; ++j) {
        const uint64_t r = ranks[j];
        if (r >= excl && r < incl) o[j] = (int32_t)i;
      }
    }
    carry += tot;
  }
}

// The aggregation's bins and stride, after the checks both entry points share.
int hist_section(const pa_query* q, int32_t agg, const uint64_t** hist, int64_t* stride) {
  if (!q || !q->prepared) return fail(PA_EINVAL, "query not prepared");
  if (const char* t = tuning_invalidating(q->tune))
    return fail(PA_EINVAL, std::string("results invalid: tuning ") + t + " is set");
  if (agg < 0 || agg >= q->spec.num_aggs || q->spec.aggs[agg].type != PA_AGG_VALUE_HISTOGRAM)
    return fail(PA_EINVAL, "not a VALUE_HISTOGRAM aggregation");
  if (q->hashed || q->agg_section[agg] < 0) return fail(PA_EINVAL, "internal: histogram without a direct key space");
  *hist = (const uint64_t*)q->sections[q->agg_section[agg]].ptr;
  *stride = hist_stride(q->spec.aggs[agg]);
  return PA_OK;
}

int hist_grow(DevBuf& b, size_t bytes) {
  if (b.n >= bytes && b.p) return PA_OK;
  dev_free(b);
  return dev_alloc(b, bytes);
}

size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// The keys pa_query_fetch returns for the current accumulators (count > 0 in ascending key order; key 0 of an
// aggregation-only query), written to q->hist_buf[0 .. num_groups): the same compaction passes as the fetch.
// `extra` bytes of q->hist_buf follow the keys (at *extra_off).
int hist_group_keys(pa_query* q, hipStream_t st, int64_t num_groups, size_t extra, size_t* extra_off) {
  const int64_t K = q->num_keys;
  const int64_t nb = (K + 2047) / 2048;
  if ((int64_t)q->fetch_blocks.n < (nb + 1) * 4) {
    dev_free(q->fetch_blocks);
    if (int rc = dev_alloc(q->fetch_blocks, (size_t)(nb + 1) * 4)) return rc;
  }
  const int all = q->spec.num_group_by != 0 ? 0 : 1;
  const unsigned long long* count = (const unsigned long long*)q->sections[0].ptr;
  uint32_t total = 0;
  PA_HIP(launch_compact(count, K, all, (uint32_t*)q->fetch_blocks.p, 0, nullptr, 0, st));
  PA_HIP(hipMemcpyAsync(&total, (uint32_t*)q->fetch_blocks.p + nb, 4, hipMemcpyDeviceToHost, st));
  PA_HIP(hipStreamSynchronize(st));
  if ((int64_t)total != num_groups)
    return fail(PA_EINVAL, "num_groups is not the group count pa_query_fetch returns for these accumulators");
  *extra_off = al256((size_t)num_groups * 8);
  if (int rc = hist_grow(q->hist_buf, *extra_off + extra)) return rc;
  if (num_groups == 0) return PA_OK;
  CompactDesc d;
  std::memset(&d, 0, sizeof(d));
  d.keys = (int64_t*)q->hist_buf.p;
  PA_HIP(launch_compact(count, K, all, (uint32_t*)q->fetch_blocks.p, num_groups, &d, 1, st));
  return PA_OK;
}

}  // namespace

extern "C" {

int64_t pa_query_fetch_histogram(pa_query* q, void* stream, int32_t agg, int64_t num_groups, int64_t capacity,
                                 int64_t* out_row_ends, int32_t* out_value_ids, int64_t* out_value_counts) {
  const uint64_t* hist = nullptr;
  int64_t stride = 0;
  if (int rc = hist_section(q, agg, &hist, &stride)) return rc;
  if (num_groups < 0 || capacity < 0 || num_groups > INT32_MAX) return fail(PA_EINVAL, "fetch histogram: bad sizes");
  if (capacity > 0 && (!out_value_ids || !out_value_counts)) return fail(PA_EINVAL, "fetch histogram: null pair arrays");
  hipStream_t st = (hipStream_t)stream;
  size_t off_at = 0;
  if (int rc = hist_group_keys(q, st, num_groups, (size_t)(num_groups + 1) * 8, &off_at)) return rc;
  if (num_groups == 0) return 0;
  const int64_t* keys = (const int64_t*)q->hist_buf.p;
  uint64_t* off = (uint64_t*)((char*)q->hist_buf.p + off_at);
  const unsigned G = (unsigned)num_groups;
  const bool wave = stride <= kHistShortRow;
  if (wave) hist_count_kernel<64><<<G, 64, 0, st>>>(hist, stride, keys, off);
  else hist_count_kernel<kHistWG><<<G, kHistWG, 0, st>>>(hist, stride, keys, off);
  hist_scan_kernel<<<1, kHistWG, 0, st>>>(off, num_groups);
  PA_HIP(hipGetLastError());
  uint64_t total = 0;
  PA_HIP(hipMemcpyAsync(&total, off + num_groups, 8, hipMemcpyDeviceToHost, st));
  if (out_row_ends)  // (the exclusive offsets shifted by one are the ends)
    PA_HIP(hipMemcpyAsync(out_row_ends, off + 1, (size_t)num_groups * 8, hipMemcpyDeviceToHost, st));
  PA_HIP(hipStreamSynchronize(st));
  const int64_t n = std::min<int64_t>((int64_t)total, capacity);
  if (n == 0) return (int64_t)total;
  const size_t counts_at = al256((size_t)n * 4);
  if (int rc = hist_grow(q->hist_pairs, counts_at + (size_t)n * 8)) return rc;
  int32_t* ids = (int32_t*)q->hist_pairs.p;
  int64_t* counts = (int64_t*)((char*)q->hist_pairs.p + counts_at);
  if (wave) hist_compact_kernel<64><<<G, 64, 0, st>>>(hist, stride, keys, off, n, ids, counts);
  else hist_compact_kernel<kHistWG><<<G, kHistWG, 0, st>>>(hist, stride, keys, off, n, ids, counts);
  PA_HIP(hipGetLastError());
  PA_HIP(hipMemcpyAsync(out_value_ids, ids, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  PA_HIP(hipMemcpyAsync(out_value_counts, counts, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  PA_HIP(hipStreamSynchronize(st));
  return (int64_t)total;
}

int pa_query_percentiles(pa_query* q, void* stream, int32_t agg, int64_t num_groups, int32_t num_percentiles,
                         const double* percentiles, int32_t* out_value_ids) {
  const uint64_t* hist = nullptr;
  int64_t stride = 0;
  if (int rc = hist_section(q, agg, &hist, &stride)) return rc;
  if (num_groups < 0 || num_groups > INT32_MAX || num_percentiles < 1 || num_percentiles > PA_MAX_PERCENTILES ||
      !percentiles || !out_value_ids)
    return fail(PA_EINVAL, "percentiles: bad arguments");
  for (int j = 0; j < num_percentiles; ++j)
    if (!(percentiles[j] >= 0.0 && percentiles[j] <= 100.0))
      return fail(PA_EINVAL, "Invalid percentile: " + std::to_string(percentiles[j]));
  hipStream_t st = (hipStream_t)stream;
  const size_t out_at = al256((size_t)PA_MAX_PERCENTILES * 8);
  size_t pct_at = 0;
  if (int rc = hist_group_keys(q, st, num_groups, out_at + (size_t)num_groups * num_percentiles * 4, &pct_at)) return rc;
  if (num_groups == 0) return PA_OK;
  const int64_t* keys = (const int64_t*)q->hist_buf.p;
  double* pct = (double*)((char*)q->hist_buf.p + pct_at);
  int32_t* out = (int32_t*)((char*)q->hist_buf.p + pct_at + out_at);
  PA_HIP(hipMemcpyAsync(pct, percentiles, (size_t)num_percentiles * 8, hipMemcpyHostToDevice, st));
  const unsigned G = (unsigned)num_groups;
  if (stride <= kHistShortRow) hist_select_kernel<64><<<G, 64, 0, st>>>(hist, stride, keys, num_percentiles, pct, out);
  else hist_select_kernel<kHistWG><<<G, kHistWG, 0, st>>>(hist, stride, keys, num_percentiles, pct, out);
  PA_HIP(hipGetLastError());
  PA_HIP(hipMemcpyAsync(out_value_ids, out, (size_t)num_groups * num_percentiles * 4, hipMemcpyDeviceToHost, st));
  PA_HIP(hipStreamSynchronize(st));
  return PA_OK;
}

}  // extern "C"
