// The finish of a PA_AGG_MOMENTS aggregation (moments_kernel, pa_moments.hip): one key's count and its
// PA_MOMENTS_WORDS accumulator words (pinot_amd.h PA_ACC_MOM_I64 / PA_ACC_MOM_F64) to the reference's tuple —
// VarianceTuple (count, sum, m2) or CovarianceTuple (sumX, sumY, sumXY, count).
//
// Portable C++ on pa_round.h: the device compiles it as __host__ __device__, and tests/native/moments_check.cpp runs
// the same bodies on the host.
#pragma once
#include "pa_round.h"

namespace pa {

// a * b of two unsigned 64-bit integers as hi:lo
PA_ROUND_HD inline void mul_u64(uint64_t a, uint64_t b, uint64_t& hi, uint64_t& lo) {
  const uint64_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
  const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
  const uint64_t mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;
  lo = (mid << 32) | (uint32_t)p00;
  hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

// Integer form, variance: n docs (< 2^32), S1 = sum x (|x| <= 2^31), the pair (hs, ls) of S2 = sum x^2 = hs * 2^32 + ls
// (< 2^94). N = n * S2 - S1^2 is exact in unsigned 128-bit arithmetic (0 <= N < 2^126: Cauchy-Schwarz below, n * S2
// above); m2 = (double)N / (double)n: N rounded once (correctly), n exact, one division.
PA_ROUND_HD inline double moments_m2_integer(uint64_t n, int64_t s1, int64_t hs, uint64_t ls) {
  if (n == 0) return 0.0;
  int64_t s2h;
  uint64_t s2l;
  sum_pair_to_i128(hs, ls, s2h, s2l);  // S2 = s2h:s2l, s2h < 2^30
  uint64_t ah, al, bh, bl, ch, cl;
  mul_u64(n, s2l, ah, al);                // n * low word
  mul_u64(n, (uint64_t)s2h, bh, bl);      // n * high word: < 2^62, so bh = 0
  ah += bl;                               // n * S2 = ah:al
  const uint64_t m = s1 < 0 ? 0ull - (uint64_t)s1 : (uint64_t)s1;  // |S1| < 2^63
  mul_u64(m, m, ch, cl);                  // S1^2
  const uint64_t nl = al - cl;
  const uint64_t nh = ah - ch - (al < cl ? 1ull : 0ull);
  return i128_to_double((int64_t)nh, nl) / (double)n;
}

// forms as in pinot_amd.h (PA_MOMENTS_FORM_INTEGER = 1, PA_MOMENTS_FORM_DOUBLE = 2)
// out: variance { sum, m2, 0 }; covariance { sumX, sumY, sumXY }. n = 0 gives zeros.
PA_ROUND_HD inline void moments_finish(int form, bool cov, double pivot, uint64_t n, const uint64_t* w, double* out) {
  out[0] = out[1] = out[2] = 0.0;
  if (n == 0) return;
  if (form == 1) {
    const int64_t s1 = (int64_t)w[0];
    out[0] = i128_to_double(s1 < 0 ? -1 : 0, (uint64_t)s1);
    if (cov) {
      const int64_t sy = (int64_t)w[1];
      out[1] = i128_to_double(sy < 0 ? -1 : 0, (uint64_t)sy);
      int64_t hi;
      uint64_t lo;
      sum_pair_to_i128((int64_t)w[3], w[2], hi, lo);
      out[2] = i128_to_double(hi, lo);
    } else {
      out[1] = moments_m2_integer(n, s1, (int64_t)w[3], w[2]);
    }
    return;
  }
  double d[3];
  for (int i = 0; i < 3; ++i) {
    // (the words' bits as doubles, without a type-punned read)
    const uint64_t b = w[i];
    double x;
    __builtin_memcpy(&x, &b, 8);
    d[i] = x;
  }
  if (cov) {
    out[0] = d[0];
    out[1] = d[1];
    out[2] = d[2];
    return;
  }
  const double dn = (double)n;
  out[0] = fma(dn, pivot, d[0]);                 // sum x = S1 + n * pivot
  const double m2 = fma(-d[0], d[0] / dn, d[2]);  // S2 - S1 * S1 / n
  out[1] = m2 < 0.0 ? 0.0 : m2;                  // (NaN stays NaN)
}

}  // namespace pa
