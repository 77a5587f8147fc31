// Fetch (gfx950 / CDNA4 only): ordered compaction of the non-empty keys and the row gather, with their launchers.
#include "pa_round.h"
#include "pa_launch.h"

namespace pa {

// out[i*per + j] = src[keys[i]*per + j] for elements of `esize` bytes (4 or 8)
__global__ void gather_kernel(const void* src, int esize, int64_t per, const int64_t* keys, int64_t n, void* out) {
  const int64_t total = n * per;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / per, j = i - r * per;
    const int64_t s = keys[r] * per + j;
    if (esize == 8) ((uint64_t*)out)[i] = ((const uint64_t*)src)[s];
    else ((uint32_t*)out)[i] = ((const uint32_t*)src)[s];
  }
}

// ---------------------------------------------------------------- fetch: ordered compaction of non-empty keys
// Block b covers keys [2048b, 2048b + 2048): thread t owns keys 8t .. 8t+7 of it.
constexpr int kCompactKeys = 2048;

__device__ __forceinline__ uint32_t block_exclusive_scan_256(uint32_t v, uint32_t* sh, uint32_t* total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const uint32_t add = t >= o ? sh[t - o] : 0u;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  const uint32_t incl = sh[t];
  if (total) *total = sh[255];
  __syncthreads();
  return incl - v;
}

__global__ void __launch_bounds__(256) compact_count_kernel(const unsigned long long* count, int64_t K, int all,
                                                            uint32_t* block_sums) {
  __shared__ uint32_t sh[256];
  const int64_t k0 = (int64_t)blockIdx.x * kCompactKeys + 8 * threadIdx.x;
  uint32_t c = 0;
  for (int j = 0; j < 8; ++j) c += (k0 + j < K) && (all || count[k0 + j] != 0);
  uint32_t total;
  block_exclusive_scan_256(c, sh, &total);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// single workgroup: in-place exclusive scan of n block sums; v[n] = total
__global__ void __launch_bounds__(256) compact_scan_kernel(uint32_t* v, int64_t n) {
  __shared__ uint32_t sh[256];
  uint32_t carry = 0;
  for (int64_t base = 0; base < n; base += 256) {
    const int64_t i = base + threadIdx.x;
    const uint32_t x = i < n ? v[i] : 0u;
    uint32_t tot;
    const uint32_t ex = block_exclusive_scan_256(x, sh, &tot);
    if (i < n) v[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) v[n] = carry;
}

__global__ void __launch_bounds__(256) compact_gather_kernel(const unsigned long long* count, int64_t K, int all,
                                                             const uint32_t* block_off, int64_t cap,
                                                             CompactDesc d) {
  __shared__ uint32_t sh[256];
  const int64_t k0 = (int64_t)blockIdx.x * kCompactKeys + 8 * threadIdx.x;
  uint32_t c = 0;
  for (int j = 0; j < 8; ++j) c += (k0 + j < K) && (all || count[k0 + j] != 0);
  int64_t pos = (int64_t)block_off[blockIdx.x] + block_exclusive_scan_256(c, sh, nullptr);
  for (int j = 0; j < 8; ++j) {
    const int64_t k = k0 + j;
    if (k >= K || !(all || count[k] != 0)) continue;
    if (pos < cap) {
      d.keys[pos] = k;
      for (int si = 0; si < d.nsec; ++si) {
        const int64_t per = d.per[si];
        if (d.es[si] == 8) {
          const uint64_t* src = (const uint64_t*)d.src[si] + k * per;
          uint64_t* dst = (uint64_t*)d.dst[si] + pos * per;
          for (int64_t e = 0; e < per; ++e) dst[e] = src[e];
        } else if (d.es[si] == 1) {  // HLL registers, one byte each (per is a power of two >= 16)
          const u32x4* src = (const u32x4*)((const uint8_t*)d.src[si] + k * per);
          u32x4* dst = (u32x4*)((uint8_t*)d.dst[si] + pos * per);
          for (int64_t e = 0; e < per / 16; ++e) dst[e] = src[e];
        } else {
          const uint32_t* src = (const uint32_t*)d.src[si] + k * per;
          uint32_t* dst = (uint32_t*)d.dst[si] + pos * per;
          for (int64_t e = 0; e < per; ++e) dst[e] = src[e];
        }
      }
    }
    ++pos;
  }
}

// Block b covers keys [2048b, 2048b + 2048) as in compact_gather_kernel; positions first (thread t counts keys 8t..8t+7,
// scans, and records each key's position in LDS), then thread t writes the rows of keys t + 256 j: consecutive threads,
// consecutive rows, 8-byte columns stored as 512-byte wave bursts.
__global__ void __launch_bounds__(256) compact_final_kernel(const unsigned long long* count, int64_t K, int all,
                                                            const uint32_t* block_off, int64_t cap, FinalDesc d) {
  __shared__ uint32_t sh[256];
  __shared__ uint32_t pos[kCompactKeys];
  const int64_t kb = (int64_t)blockIdx.x * kCompactKeys;
  const int64_t k0 = kb + 8 * threadIdx.x;
  uint32_t c = 0;
  for (int j = 0; j < 8; ++j) c += (k0 + j < K) && (all || count[k0 + j] != 0);
  uint32_t p = block_exclusive_scan_256(c, sh, nullptr);
  for (int j = 0; j < 8; ++j) {
    const bool on = (k0 + j < K) && (all || count[k0 + j] != 0);
    pos[8 * threadIdx.x + j] = on ? p : 0xffffffffu;
    p += on ? 1u : 0u;
  }
  __syncthreads();
  const int64_t base = block_off[blockIdx.x];
  for (int j = 0; j < kCompactKeys / 256; ++j) {
    const int kl = threadIdx.x + 256 * j;
    const uint32_t pl = pos[kl];
    if (pl == 0xffffffffu) continue;
    const int64_t r = base + pl;
    if (r >= cap) continue;
    const int64_t k = kb + kl;
    const unsigned long long cnt = count[k];
    d.keys[r] = k;
    d.counts[r] = (int64_t)cnt;
    for (int a = 0; a < d.nagg; ++a) {
      const int t = d.type[a];
      if (t == PA_AGG_VALUE_HISTOGRAM) continue;  // 0 bytes per row (pa_query_fetch_histogram reads the bins)
      if (is_trow_agg(t)) continue;               // 0 bytes per row (pa_query_fetch_time_rows reads the rows)
      if (t == PA_AGG_DISTINCTCOUNTHLL || t == PA_AGG_DISTINCTCOUNT) {
        const int64_t per = d.per[a];  // (a multiple of 16 bytes)
        const u32x4* src = (const u32x4*)((const uint8_t*)d.sec[a] + k * per);
        u32x4* dst = (u32x4*)((uint8_t*)d.out[a] + r * per);
        for (int64_t e = 0; e < per / 16; ++e) dst[e] = src[e];
        continue;
      }
      double v;
      if (t == PA_AGG_COUNT) {
        v = (double)cnt;
      } else if (t == PA_AGG_SUM || t == PA_AGG_COUNT_MV) {
        const int64_t* sv = (const int64_t*)d.sec[a];
        if (d.src[a] == SRC_LONG) {  // exact 96-bit total hi * 2^32 + lo, rounded once
          const int64_t hs = sv[2 * k + 1];
          const uint64_t ls = (uint64_t)sv[2 * k];
          int64_t hi;
          uint64_t lo;
          sum_pair_to_i128(hs, ls, hi, lo);
          v = i128_to_double(hi, lo);
        } else if (d.src[a] == SRC_INT || t == PA_AGG_COUNT_MV) {
          v = i128_to_double(sv[k] >> 63, (uint64_t)sv[k]);
        } else {
          v = ((const double*)d.sec[a])[k];
        }
      } else {  // MIN / MAX (an empty aggregation-only result: +/-inf, Min/MaxAggregationFunction DEFAULT_VALUE)
        const int64_t e8 = ((const int64_t*)d.sec[a])[k];
        if (cnt == 0) v = t == PA_AGG_MIN ? __builtin_inf() : -__builtin_inf();
        else v = d.src[a] != SRC_DOUBLE ? i128_to_double(e8 >> 63, (uint64_t)e8) : f64_order_decode(e8);
      }
      ((double*)d.out[a])[r] = v;
    }
  }
}

hipError_t launch_compact_final(const unsigned long long* count, int64_t K, int all, const uint32_t* block_off,
                                int64_t cap, const FinalDesc* d, hipStream_t s) {
  const int64_t nb = (K + kCompactKeys - 1) / kCompactKeys;
  compact_final_kernel<<<(unsigned)nb, 256, 0, s>>>(count, K, all, block_off, cap, *d);
  return hipGetLastError();
}

hipError_t launch_compact(const unsigned long long* count, int64_t K, int all, uint32_t* block_sums, int64_t cap,
                          const CompactDesc* d, int phase, hipStream_t s) {
  const int64_t nb = (K + kCompactKeys - 1) / kCompactKeys;
  if (phase == 0) {
    compact_count_kernel<<<(unsigned)nb, 256, 0, s>>>(count, K, all, block_sums);
    compact_scan_kernel<<<1, 256, 0, s>>>(block_sums, nb);
  } else {
    compact_gather_kernel<<<(unsigned)nb, 256, 0, s>>>(count, K, all, block_sums, cap, *d);
  }
  return hipGetLastError();
}

hipError_t launch_gather(const void* src, int esize, int64_t per, const int64_t* keys, int64_t n, void* out,
                         hipStream_t s) {
  gather_kernel<<<grid_for(n * per, 256), 256, 0, s>>>(src, esize, per, keys, n, out);
  return hipGetLastError();
}

}  // namespace pa
