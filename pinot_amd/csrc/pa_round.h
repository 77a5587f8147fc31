// The final rounding of the integer accumulators (compact_final_kernel): the (high, low) pair of an exact 96-bit SUM
// back to one signed 128-bit integer, and that integer to the nearest double, with integer operations only.
//
// Portable C++: the device compiles it as __host__ __device__, and tests/native/round_check.cpp runs the same bodies on
// the host against the compiler's __int128.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PA_ROUND_HD __host__ __device__
#else
#define PA_ROUND_HD
#endif

namespace pa {

// Correctly rounded (nearest, ties to even) double of the signed 128-bit integer hi:lo — the host's (double)__int128 of
// an exact 96-bit SUM (PA_ACC_SUM_I64X2), an int64 SUM or an integer MIN / MAX, computed with integer operations only.
PA_ROUND_HD inline double i128_to_double(int64_t hi, uint64_t lo) {
  const bool neg = hi < 0;
  uint64_t mh = (uint64_t)hi, ml = lo;
  if (neg) {
    ml = ~ml + 1ull;
    mh = ~mh + (ml == 0 ? 1ull : 0ull);
  }
  if (mh == 0 && ml < (1ull << 53)) return neg ? -(double)ml : (double)ml;  // (exact)
  const int msb = mh ? 127 - __builtin_clzll(mh) : 63 - __builtin_clzll(ml);
  const int s = msb - 52;  // bits below the 53-bit significand (>= 1 here)
  auto bit = [&](int i) -> uint64_t { return i >= 64 ? (mh >> (i - 64)) & 1ull : (ml >> i) & 1ull; };
  uint64_t sig = s >= 64 ? mh >> (s - 64) : ((ml >> s) | (mh << (64 - s)));
  sig &= (1ull << 53) - 1ull;
  sig |= 1ull << 52;  // (the leading bit; the masks above keep exactly 53 bits)
  const uint64_t half = bit(s - 1);
  bool sticky;
  const int t = s - 1;  // bits [0, t) below the half bit
  if (t <= 0) sticky = false;
  else if (t >= 64) sticky = ml != 0 || (t > 64 && (mh & ((1ull << (t - 64)) - 1ull)) != 0);
  else sticky = (ml & ((1ull << t) - 1ull)) != 0;
  int e = s;
  if (half && (sticky || (sig & 1ull))) {
    ++sig;
    if (sig == (1ull << 53)) {
      sig >>= 1;
      ++e;
    }
  }
  const double d = ldexp((double)sig, e);
  return neg ? -d : d;
}

// The exact SUM of LONG values is kept as two 64-bit partial sums: ls of the values' low 32 bits (unsigned) and hs of
// their high 32 bits (signed); the total is hs * 2^32 + ls. hi:lo is that total as one signed 128-bit integer.
PA_ROUND_HD inline void sum_pair_to_i128(int64_t hs, uint64_t ls, int64_t& hi, uint64_t& lo) {
  const uint64_t l0 = (uint64_t)hs << 32;
  lo = l0 + ls;
  hi = (hs >> 32) + (lo < l0 ? 1 : 0);
}

}  // namespace pa
