// Group trim (gfx950 / CDNA4 only): ORDER BY ... LIMIT over a direct key space without moving every group — the order
// words of the candidate groups, an MSB radix select of the `trim` smallest word strings, and the gather of the kept
// groups' rows into the fetch staging layout. The device side of pa_query_fetch_trimmed (pa_fetch.hip).
//
// Order words (reduce._order_key_fn as unsigned words, most significant first): a group-by column's table-wide id; the
// 64-bit count; the final double of a SUM / MIN / MAX exactly as the fetch produces it (-0.0 first mapped to +0.0, then
// the order-preserving transform); AVG = that sum / count and MINMAXRANGE = max - min in IEEE double (this unit is built
// without fast-math); DESC complements the word. The last word is the key with group-by column 0 most significant, so
// the order is total. NaN term values are out of scope: the host comparator is no total order over them.
#include "pa_round.h"
#include "pa_launch.h"

namespace pa {

// The final double of aggregation a (COUNT / SUM / COUNT_MV / MIN / MAX) of key k: compact_final_kernel's value.
__device__ __forceinline__ double trim_final_double(const FinalDesc& d, int a, int64_t k, unsigned long long cnt) {
  const int t = d.type[a];
  if (t == PA_AGG_COUNT) return (double)cnt;
  if (t == PA_AGG_SUM || t == PA_AGG_COUNT_MV) {
    const int64_t* sv = (const int64_t*)d.sec[a];
    if (d.src[a] == SRC_LONG) {  // exact 96-bit total hi * 2^32 + lo, rounded once
      int64_t hi;
      uint64_t lo;
      sum_pair_to_i128(sv[2 * k + 1], (uint64_t)sv[2 * k], hi, lo);
      return i128_to_double(hi, lo);
    }
    if (d.src[a] == SRC_INT || t == PA_AGG_COUNT_MV) return i128_to_double(sv[k] >> 63, (uint64_t)sv[k]);
    return ((const double*)d.sec[a])[k];
  }
  const int64_t e8 = ((const int64_t*)d.sec[a])[k];  // MIN / MAX
  if (cnt == 0) return t == PA_AGG_MIN ? __builtin_inf() : -__builtin_inf();
  return d.src[a] != SRC_DOUBLE ? i128_to_double(e8 >> 63, (uint64_t)e8) : f64_order_decode(e8);
}

// double -> unsigned word of the same order (-0.0 ties with +0.0, as the host's a != b)
__device__ __forceinline__ uint64_t trim_double_word(double v) {
  if (v == 0.0) v = 0.0;
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : b | (1ull << 63);
}

__global__ void __launch_bounds__(256) trim_words_kernel(const unsigned long long* __restrict__ count,
                                                         const int64_t* __restrict__ keys, int64_t n, FinalDesc f,
                                                         TrimWordsDesc w) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t k = keys[i];
    const unsigned long long cnt = count[k];
    int64_t rem = k;
    uint64_t tie = 0;
    for (int j = 0; j < w.ngb; ++j) {  // digit j of the key has weight prod card_k, k < j; the tie word reverses that
      tie = tie * (uint64_t)w.card[j] + (uint64_t)(rem % w.card[j]);
      rem /= w.card[j];
    }
    for (int e = 0; e < w.nterms; ++e) {
      uint64_t x;
      switch (w.kind[e]) {
        case PA_TRIM_KEY_COLUMN: x = (uint64_t)((k / w.kstride[e]) % w.kcard[e]); break;
        case PA_TRIM_COUNT: x = cnt; break;
        case PA_TRIM_AGG: x = trim_double_word(trim_final_double(f, w.a[e], k, cnt)); break;
        case PA_TRIM_AVG: x = trim_double_word(trim_final_double(f, w.a[e], k, cnt) / (double)cnt); break;
        default:  // PA_TRIM_RANGE
          x = trim_double_word(trim_final_double(f, w.a[e], k, cnt) - trim_final_double(f, w.b[e], k, cnt));
          break;
      }
      w.words[(int64_t)e * n + i] = w.desc[e] ? ~x : x;
    }
    w.words[(int64_t)w.nterms * n + i] = tie;
  }
}

__global__ void trim_init_kernel(TrimCtl* ctl, unsigned long long trim) {
  if (threadIdx.x == 0 && blockIdx.x == 0) ctl->k = trim;
}

constexpr uint8_t kTrimUndecided = 0, kTrimIn = 1, kTrimOut = 2;

// One digit pass. Every workgroup first applies the previous pass's pick to the states it visits, then counts the
// digits of the still undecided candidates in an LDS histogram (a wave whose undecided lanes share one digit — the high
// bytes of counts, sign and exponent of sums — adds its popcount once) and flushes it to `hist`. The last workgroup to
// flush picks the bin that holds rank k with its first wave.
__global__ void __launch_bounds__(256) trim_pass_kernel(const uint64_t* __restrict__ words, int shift, int pass,
                                                        int64_t n, uint8_t* __restrict__ state,
                                                        uint32_t* __restrict__ hist, TrimCtl* ctl) {
  __shared__ uint32_t lh[256];
  __shared__ int is_last;
  // (the control block is written by a pass's last workgroup only after every workgroup of that pass took its ticket,
  // which each does after these reads)
  if (ctl->done) return;
  const int pending = ctl->pending;
  const uint64_t* pw = ctl->pend_words;
  const int pshift = ctl->pend_shift, pbin = ctl->pend_bin;
  const int t = threadIdx.x, lane = t & 63;
  lh[t] = 0;
  __syncthreads();
  for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + t;
    bool und = false;
    uint32_t dg = 0;
    if (i < n && state[i] == kTrimUndecided) {
      und = true;
      if (pending) {
        const int pd = (int)((pw[i] >> pshift) & 255);
        if (pd != pbin) {
          state[i] = pd < pbin ? kTrimIn : kTrimOut;
          und = false;
        }
      }
      if (und) dg = (uint32_t)((words[i] >> shift) & 255);
    }
    const unsigned long long m = __ballot(und);
    if (m) {
      const int first = __ffsll(m) - 1;
      const uint32_t d0 = (uint32_t)__shfl((int)dg, first);
      if (__all(!und || dg == d0)) {
        if (lane == first) atomicAdd(&lh[d0], (uint32_t)__popcll(m));
      } else if (und) {
        atomicAdd(&lh[dg], 1u);
      }
    }
  }
  __syncthreads();
  uint32_t* h = hist + (int64_t)pass * 256;
  if (lh[t]) atomicAdd(&h[t], lh[t]);
  __threadfence();
  __syncthreads();
  if (t == 0) is_last = atomicAdd(&ctl->ticket[pass], 1u) == gridDim.x - 1;
  __syncthreads();
  if (!is_last) return;
  __threadfence();
  lh[t] = __hip_atomic_load(&h[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (t >= 64) return;
  uint32_t hb[4];
  uint32_t s = 0;
  for (int j = 0; j < 4; ++j) {
    hb[j] = lh[4 * t + j];
    s += hb[j];
  }
  unsigned long long inc = s;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long up = (unsigned long long)__shfl_up((long long)inc, o);
    if (t >= o) inc += up;
  }
  const unsigned long long total = (unsigned long long)__shfl((long long)inc, 63);
  const unsigned long long exc = inc - s;
  const unsigned long long k = ctl->k;
  if (k == 0 || k >= total) {  // the class is not needed at all, or needed whole
    if (t == 0) {
      ctl->pending = 0;
      ctl->rest_in = k != 0;
      ctl->done = 1;
    }
    return;
  }
  if (exc < k && k <= inc) {  // exactly one lane
    unsigned long long c = exc;
    for (int j = 0; j < 4; ++j) {
      if (k <= c + hb[j]) {
        ctl->pend_words = words;
        ctl->pend_shift = shift;
        ctl->pend_bin = 4 * t + j;
        ctl->pending = 1;
        ctl->k = k - c;
        if (k - c == hb[j]) {  // the bin is needed whole
          ctl->rest_in = 1;
          ctl->done = 1;
        }
        break;
      }
      c += hb[j];
    }
  }
}

// flag[i] = candidate i is kept: its state, with the last pick and the fate of the undecided class applied
__global__ void __launch_bounds__(256) trim_mark_kernel(const uint8_t* __restrict__ state, int64_t n,
                                                        const TrimCtl* __restrict__ ctl,
                                                        unsigned long long* __restrict__ flag) {
  const int pending = ctl->pending, rest_in = ctl->rest_in;
  const uint64_t* pw = ctl->pend_words;
  const int pshift = ctl->pend_shift, pbin = ctl->pend_bin;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const uint8_t s = state[i];
    bool in = s == kTrimIn;
    if (s == kTrimUndecided) {
      in = rest_in != 0;
      if (pending) {
        const int pd = (int)((pw[i] >> pshift) & 255);
        if (pd != pbin) in = pd < pbin;
      }
    }
    flag[i] = in ? 1ull : 0ull;
  }
}

// Row r of the staging columns from candidate sel[r]: compact_final_kernel's row, for the kept groups only.
__global__ void __launch_bounds__(256) trim_rows_kernel(const unsigned long long* __restrict__ count,
                                                        const int64_t* __restrict__ keys,
                                                        const int64_t* __restrict__ sel, int64_t n, int64_t m,
                                                        FinalDesc d) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < m; r += (int64_t)gridDim.x * 256) {
    const int64_t i = sel[r];
    if ((uint64_t)i >= (uint64_t)n) continue;  // (a row the select did not fill: the caller checks the kept count)
    const int64_t k = keys[i];
    const unsigned long long cnt = count[k];
    d.keys[r] = k;
    d.counts[r] = (int64_t)cnt;
    for (int a = 0; a < d.nagg; ++a) {
      const int t = d.type[a];
      if (t == PA_AGG_VALUE_HISTOGRAM) continue;
      if (t == PA_AGG_DISTINCTCOUNTHLL || t == PA_AGG_DISTINCTCOUNT) {
        const int64_t per = d.per[a];  // (a multiple of 16 bytes)
        const u32x4* src = (const u32x4*)((const uint8_t*)d.sec[a] + k * per);
        u32x4* dst = (u32x4*)((uint8_t*)d.out[a] + r * per);
        for (int64_t e = 0; e < per / 16; ++e) dst[e] = src[e];
        continue;
      }
      ((double*)d.out[a])[r] = trim_final_double(d, a, k, cnt);
    }
  }
}

hipError_t launch_trim_words(const unsigned long long* count, const FinalDesc* f, const TrimWordsDesc* w,
                             const int64_t* keys, int64_t n, hipStream_t s) {
  trim_words_kernel<<<grid_for(n, 256), 256, 0, s>>>(count, keys, n, *f, *w);
  return hipGetLastError();
}

hipError_t launch_trim_select(const TrimPlan* p, int64_t trim, hipStream_t s) {
  hipError_t e = hipMemsetAsync(p->state, 0, (size_t)p->n, s);
  if (e == hipSuccess) e = hipMemsetAsync(p->hist, 0, (size_t)kTrimMaxPasses * 256 * 4, s);
  if (e == hipSuccess) e = hipMemsetAsync(p->ctl, 0, sizeof(TrimCtl), s);
  if (e != hipSuccess) return e;
  trim_init_kernel<<<1, 64, 0, s>>>(p->ctl, (unsigned long long)trim);
  const int grid = grid_for(p->n, 256);
  for (int i = 0; i < p->npass; ++i)
    trim_pass_kernel<<<grid, 256, 0, s>>>(p->words + (int64_t)p->word[i] * p->n, p->shift[i], i, p->n, p->state,
                                          p->hist, p->ctl);
  trim_mark_kernel<<<grid, 256, 0, s>>>(p->state, p->n, p->ctl, p->flag);
  return hipGetLastError();
}

hipError_t launch_trim_rows(const unsigned long long* count, const int64_t* keys, const int64_t* sel, int64_t n,
                            int64_t m, const FinalDesc* d, hipStream_t s) {
  trim_rows_kernel<<<grid_for(m, 256), 256, 0, s>>>(count, keys, sel, n, m, *d);
  return hipGetLastError();
}

}  // namespace pa
