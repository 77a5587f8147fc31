// Segment-load and query-prep kernels (gfx950 / CDNA4 only): byte swap, HLL look-up tables, fill and reset, with their
// launchers.
#include "pa_launch.h"

namespace pa {

__global__ void bswap_words_kernel(uint32_t* w, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    w[i] = __builtin_bswap32(w[i]);
}

// dictId -> (register << 8) | rank for DISTINCTCOUNTHLL over a dictionary column.
// MurmurHash.hash(Object) on the boxed dictionary value (Dictionary.get): Integer/Long -> hashLong(v),
// Float -> hashLong(Float.floatToRawIntBits(v)), Double -> hashLong(Double.doubleToRawLongBits(v)).
__global__ void hll_lut_numeric_kernel(const int64_t* di, const double* dd, int32_t vtype, int32_t card,
                                       int32_t log2m, uint32_t* lut) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < card; i += gridDim.x * blockDim.x) {
    int64_t x;
    switch (vtype) {
      case PA_INT: case PA_LONG: x = di[i]; break;
      case PA_FLOAT: x = __builtin_bit_cast(int32_t, (float)dd[i]); break;
      default: x = __builtin_bit_cast(int64_t, dd[i]); break;
    }
    lut[i] = hll_slot_rank(murmur_hash_long(x), log2m);
  }
}

__global__ void hll_lut_hashes_kernel(const int32_t* hashes, int32_t card, int32_t log2m, uint32_t* lut) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < card; i += gridDim.x * blockDim.x)
    lut[i] = hll_slot_rank(hashes[i], log2m);
}

__global__ void fill_i64_kernel(int64_t* p, int64_t n, int64_t v) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}

// Word i of the block followed by the header: the identity of the section holding it, else zero. One store per word,
// so the zeroing and the identities cannot race.
__global__ void __launch_bounds__(256) reset_kernel(ResetArgs a) {
  const int64_t total = a.block_words + a.header_words;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    if (i >= a.block_words) {
      a.header[i - a.block_words] = 0;
      continue;
    }
    int64_t v = 0;
    for (int k = 0; k < a.num_sections; ++k)
      if ((uint64_t)(i - a.sec[k].first) < (uint64_t)a.sec[k].n) v = a.sec[k].value;
    a.block[i] = v;
  }
}

hipError_t launch_bswap_words(uint32_t* w, int64_t n, hipStream_t s) {
  bswap_words_kernel<<<grid_for(n, 256), 256, 0, s>>>(w, n);
  return hipGetLastError();
}

hipError_t launch_hll_lut_numeric(const int64_t* di, const double* dd, int32_t vtype, int32_t card, int32_t log2m,
                                  uint32_t* lut, hipStream_t s) {
  hll_lut_numeric_kernel<<<grid_for(card, 256), 256, 0, s>>>(di, dd, vtype, card, log2m, lut);
  return hipGetLastError();
}

hipError_t launch_hll_lut_hashes(const int32_t* hashes, int32_t card, int32_t log2m, uint32_t* lut, hipStream_t s) {
  hll_lut_hashes_kernel<<<grid_for(card, 256), 256, 0, s>>>(hashes, card, log2m, lut);
  return hipGetLastError();
}

hipError_t launch_fill_i64(int64_t* p, int64_t n, int64_t v, hipStream_t s) {
  fill_i64_kernel<<<grid_for(n, 256), 256, 0, s>>>(p, n, v);
  return hipGetLastError();
}

hipError_t launch_reset(const ResetArgs& a, hipStream_t s) {
  reset_kernel<<<grid_for(a.block_words + a.header_words, 256), 256, 0, s>>>(a);
  return hipGetLastError();
}

}  // namespace pa
