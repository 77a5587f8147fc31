// PA_AGG_MOMENTS results (PA_ACC_MOM_I64 / PA_ACC_MOM_F64: PA_MOMENTS_WORDS words per key): pa_query_fetch_moments,
// the reference's VarianceTuple / CovarianceTuple of every fetched group as columns. One thread per fetched group
// finishes its tuple from the group's count and words (pa_moments_finish.h); one copy per column.
#include "pa_host.h"
#include "pa_moments_finish.h"

namespace {

constexpr int kMomThreads = 256;

__global__ void __launch_bounds__(kMomThreads)
    moments_kernel(const unsigned long long* __restrict__ count, const uint64_t* __restrict__ words,
                   const int64_t* __restrict__ keys, int64_t n, int form, int cov, double pivot,
                   int64_t* __restrict__ out_count, double* __restrict__ out_values) {
  for (int64_t g = (int64_t)blockIdx.x * kMomThreads + threadIdx.x; g < n; g += (int64_t)gridDim.x * kMomThreads) {
    const int64_t k = keys[g];
    const uint64_t c = count[k];
    uint64_t w[PA_MOMENTS_WORDS];
#pragma unroll
    for (int i = 0; i < PA_MOMENTS_WORDS; ++i) w[i] = words[k * PA_MOMENTS_WORDS + i];
    double o[3];
    pa::moments_finish(form, cov != 0, pivot, c, w, o);
    out_count[g] = (int64_t)c;
    out_values[g] = o[0];
    out_values[n + g] = o[1];
    out_values[2 * n + g] = o[2];
  }
}

}  // namespace

using namespace pa;

extern "C" {

int pa_query_fetch_moments(pa_query* q, void* stream, int32_t agg, int64_t num_groups, int64_t* out_count,
                           double* const* out_values) {
  if (!q || !q->prepared) return fail(PA_EINVAL, "query not prepared");
  if (const char* t = tuning_invalidating(q->tune))
    return fail(PA_EINVAL, std::string("results invalid: tuning ") + t + " is set");
  if (agg < 0 || agg >= q->spec.num_aggs || !q->mom_form[agg]) return fail(PA_EINVAL, "not a PA_AGG_MOMENTS aggregation");
  if (q->hashed || q->agg_section[agg] < 0) return fail(PA_EINVAL, "internal: moments without a direct key space");
  if (num_groups < 0 || num_groups > INT32_MAX) return fail(PA_EINVAL, "fetch moments: bad sizes");
  hipStream_t st = (hipStream_t)stream;
  // the keys pa_query_fetch returns for these accumulators: the same compaction passes
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
  if (num_groups == 0) return PA_OK;
  // keys | counts | values [3][group]
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t n = (size_t)num_groups;
  const size_t o_cnt = al(n * 8), o_val = o_cnt + al(n * 8);
  const size_t bytes = o_val + al(n * 3 * 8);
  if (q->mom_buf.n < bytes || !q->mom_buf.p) {
    dev_free(q->mom_buf);
    if (int rc = dev_alloc(q->mom_buf, bytes)) return rc;
  }
  char* b = (char*)q->mom_buf.p;
  CompactDesc d;
  std::memset(&d, 0, sizeof(d));
  d.keys = (int64_t*)b;
  PA_HIP(launch_compact(count, K, all, (uint32_t*)q->fetch_blocks.p, num_groups, &d, 1, st));
  hipLaunchKernelGGL(moments_kernel, dim3((unsigned)std::min<int64_t>(1024, (num_groups + kMomThreads - 1) / kMomThreads)),
                     dim3(kMomThreads), 0, st, count, (const uint64_t*)q->sections[q->agg_section[agg]].ptr,
                     (const int64_t*)b, num_groups, q->mom_form[agg], q->mom_slot2[agg] >= 0 ? 1 : 0, q->mom_pivot[agg],
                     (int64_t*)(b + o_cnt), (double*)(b + o_val));
  PA_HIP(hipGetLastError());
  if (out_count) PA_HIP(hipMemcpyAsync(out_count, b + o_cnt, n * 8, hipMemcpyDeviceToHost, st));
  for (int c = 0; c < 3; ++c)
    if (out_values && out_values[c])
      PA_HIP(hipMemcpyAsync(out_values[c], b + o_val + (size_t)c * n * 8, n * 8, hipMemcpyDeviceToHost, st));
  PA_HIP(hipStreamSynchronize(st));
  return PA_OK;
}

}  // extern "C"
