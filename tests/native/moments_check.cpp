// Host check of csrc/pa_moments_finish.h (the finish arithmetic of PA_AGG_MOMENTS, compiled for the device as
// __host__ __device__): the same bodies on the host against the compiler's __int128 arithmetic and std::fma.
//
//   mul_u64            against unsigned __int128 products
//   moments_m2_integer N = n * S2 - S1^2 against unsigned __int128, m2 == (double)N / (double)n bit for bit, over columns
//                      of INT32_MIN / INT32_MAX / alternating / random int32 values with up to 2^32 - 1 docs (the words
//                      built as the scan builds them: low-32 and high-32 sums of the squares)
//   moments_finish     the integer covariance sums against (double)__int128, the double form's fma expressions, n = 0
//
// Prints "<set> cases=<n> mismatches=<m>" per set and a TOTAL line; exit status 1 on any mismatch.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <random>

#include "pa_moments_finish.h"

typedef unsigned __int128 u128;
typedef __int128 i128;

static uint64_t bits(double d) {
  uint64_t b;
  std::memcpy(&b, &d, 8);
  return b;
}

struct Tally {
  const char* name;
  long cases = 0, bad = 0;
  void check(bool ok, const char* what) {
    ++cases;
    if (!ok) {
      ++bad;
      if (bad <= 5) std::fprintf(stderr, "MISMATCH %s: %s\n", name, what);
    }
  }
};

// n docs: `a` docs of value x and n - a docs of value y (exact sums in 128 bits), as the scan's words
static void words_of(uint64_t a, int64_t x, uint64_t b, int64_t y, uint64_t w[4], u128* s2_out, i128* s1_out) {
  const i128 s1 = (i128)a * x + (i128)b * y;
  const u128 px = (u128)((i128)x * x), py = (u128)((i128)y * y);
  const u128 lo = (u128)a * (uint64_t)(uint32_t)(uint64_t)px + (u128)b * (uint64_t)(uint32_t)(uint64_t)py;
  const u128 hi = (u128)a * (uint64_t)(px >> 32) + (u128)b * (uint64_t)(py >> 32);
  w[0] = (uint64_t)(int64_t)s1;
  w[1] = 0;
  w[2] = (uint64_t)lo;  // (n < 2^32 docs: the low-32 sum stays below 2^64)
  w[3] = (uint64_t)hi;
  *s2_out = (u128)a * px + (u128)b * py;
  *s1_out = s1;
}

int main() {
  std::mt19937_64 rng(12345);
  long total = 0, total_bad = 0;
  auto done = [&](const Tally& t) {
    std::printf("%s cases=%ld mismatches=%ld\n", t.name, t.cases, t.bad);
    total += t.cases;
    total_bad += t.bad;
  };

  Tally mul{"mul_u64"};
  for (int i = 0; i < 200000; ++i) {
    uint64_t a = rng(), b = rng();
    if (i % 7 == 0) a = ~0ull;
    if (i % 11 == 0) b = ~0ull;
    if (i % 13 == 0) a >>= (rng() % 64);
    uint64_t hi, lo;
    pa::mul_u64(a, b, hi, lo);
    const u128 p = (u128)a * b;
    mul.check(hi == (uint64_t)(p >> 64) && lo == (uint64_t)p, "product");
  }
  done(mul);

  Tally m2{"m2_integer"};
  const int64_t lim[] = {INT32_MIN, INT32_MAX, INT32_MIN + 1, -1, 0, 1, 12345, -500};
  const uint64_t counts[] = {1, 2, 3, 4, 6144, 6149, 65536, 1000003, 2147483647ull, 4294967295ull};
  auto one = [&](uint64_t a, int64_t x, uint64_t b, int64_t y) {
    const uint64_t n = a + b;
    if (n == 0 || n > 4294967295ull) return;
    uint64_t w[4];
    u128 s2;
    i128 s1;
    words_of(a, x, b, y, w, &s2, &s1);
    const u128 N = (u128)n * s2 - (u128)(s1 * s1);
    const double want = (double)N / (double)n;
    const double got = pa::moments_m2_integer(n, (int64_t)w[0], (int64_t)w[3], w[2]);
    m2.check(bits(got) == bits(want), "m2");
    double out[3];
    pa::moments_finish(1, false, 0.0, n, w, out);
    m2.check(bits(out[0]) == bits((double)s1) && bits(out[1]) == bits(want) && out[2] == 0.0, "finish variance");
  };
  for (int64_t x : lim)
    for (int64_t y : lim)
      for (uint64_t a : counts)
        for (uint64_t b : counts) one(a, x, b, y);
  for (int i = 0; i < 300000; ++i) {
    const int64_t x = (int64_t)(int32_t)rng(), y = (int64_t)(int32_t)rng();
    const uint64_t a = rng() >> (33 + rng() % 31), b = rng() >> (33 + rng() % 31);
    one(a, x, b, y);
  }
  done(m2);

  Tally cov{"covariance_integer"};
  for (int i = 0; i < 300000; ++i) {
    // n docs of (x, y): the words of the sums of x, y and the split product
    const int64_t x = i % 5 == 0 ? INT32_MIN : (int64_t)(int32_t)rng();
    const int64_t y = i % 3 == 0 ? INT32_MAX : (i % 7 == 0 ? INT32_MIN : (int64_t)(int32_t)rng());
    const uint64_t n = 1 + (rng() >> (32 + rng() % 32));
    const i128 p = (i128)x * y;
    const i128 lo = (i128)n * (uint64_t)(uint32_t)(uint64_t)p, hi = (i128)n * (int64_t)(p >> 32);
    uint64_t w[4] = {(uint64_t)(int64_t)((i128)n * x), (uint64_t)(int64_t)((i128)n * y), (uint64_t)lo, (uint64_t)(int64_t)hi};
    double out[3];
    pa::moments_finish(1, true, 0.0, n, w, out);
    cov.check(bits(out[0]) == bits((double)((i128)n * x)) && bits(out[1]) == bits((double)((i128)n * y)) &&
                  bits(out[2]) == bits((double)((i128)n * p)),
              "sums");
  }
  done(cov);

  Tally dbl{"double_form"};
  std::uniform_real_distribution<double> U(-1e6, 1e6);
  for (int i = 0; i < 200000; ++i) {
    const double s1 = U(rng), s2 = std::fabs(U(rng)) * 1e3, sy = U(rng), pivot = i % 4 == 0 ? 1e9 : U(rng);
    const uint64_t n = 1 + rng() % 100000;
    uint64_t w[4] = {bits(s1), bits(sy), bits(s2), 0};
    double out[3];
    pa::moments_finish(2, false, pivot, n, w, out);
    const double dn = (double)n;
    double m = std::fma(-s1, s1 / dn, s2);
    if (m < 0.0) m = 0.0;
    dbl.check(bits(out[0]) == bits(std::fma(dn, pivot, s1)) && bits(out[1]) == bits(m) && out[2] == 0.0, "variance");
    pa::moments_finish(2, true, 0.0, n, w, out);
    dbl.check(bits(out[0]) == bits(s1) && bits(out[1]) == bits(sy) && bits(out[2]) == bits(s2), "covariance");
    pa::moments_finish(i % 2 + 1, i % 3 == 0, pivot, 0, w, out);
    dbl.check(out[0] == 0.0 && out[1] == 0.0 && out[2] == 0.0, "no docs");
  }
  {  // NaN stays NaN through the clamp
    uint64_t w[4] = {bits(1.0), 0, bits(std::nan("")), 0};
    double out[3];
    pa::moments_finish(2, false, 0.0, 3, w, out);
    dbl.check(out[1] != out[1], "nan");
  }
  done(dbl);

  std::printf("TOTAL cases=%ld mismatches=%ld\n", total, total_bad);
  return total_bad ? 1 : 0;
}
