// Stand-alone check of pa::i128_to_double and pa::sum_pair_to_i128 (pinot_amd/csrc/pa_round.h) against the compiler's
// __int128: the double bit for bit with (double)(__int128), the recombination with ((__int128)hs << 32) + ls.
// Prints one line "<set> cases=.. mismatches=.." per input set and "TOTAL ..." at the end; exit status 1 when any
// case differs.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "pa_round.h"

namespace {

typedef __int128 i128;
typedef unsigned __int128 u128;

struct Rng {  // xorshift64*
  uint64_t s;
  uint64_t next() {
    s ^= s >> 12;
    s ^= s << 25;
    s ^= s >> 27;
    return s * 0x2545F4914F6CDD1Dull;
  }
};

struct Set {
  const char* name;
  long cases = 0, bad = 0;
  explicit Set(const char* n) : name(n) {}
  void print() const { std::printf("%s cases=%ld mismatches=%ld\n", name, cases, bad); }
};

uint64_t bits_of(double d) {
  uint64_t u;
  std::memcpy(&u, &d, 8);
  return u;
}

void report(const char* what, i128 v, uint64_t got, uint64_t want) {
  std::fprintf(stderr, "MISMATCH %s hi=%lld lo=%llu got=%016llx want=%016llx\n", what, (long long)(int64_t)(v >> 64),
               (unsigned long long)(uint64_t)v, (unsigned long long)got, (unsigned long long)want);
}

// one value: the header's double against the compiler's
void check_round(Set& s, i128 v) {
  const uint64_t got = bits_of(pa::i128_to_double((int64_t)(v >> 64), (uint64_t)v));
  const uint64_t want = bits_of((double)v);
  ++s.cases;
  if (got != want) {
    if (++s.bad <= 10) report(s.name, v, got, want);
  }
}

void check_round_both(Set& s, i128 v) {
  check_round(s, v);
  check_round(s, -v);
}

// one pair of partial sums: the recombination against 128-bit arithmetic, then the rounding of the total
void check_pair(Set& s, int64_t hs, uint64_t ls) {
  int64_t hi;
  uint64_t lo;
  pa::sum_pair_to_i128(hs, ls, hi, lo);
  const i128 want = (i128)((u128)(i128)hs << 32) + (i128)(u128)ls;  // (the shift on the unsigned type: no UB)
  const i128 got = (i128)(((u128)(uint64_t)hi << 64) | (u128)lo);
  ++s.cases;
  if (got != want) {
    if (++s.bad <= 10) report(s.name, want, (uint64_t)hi, (uint64_t)(want >> 64));
  }
  check_round(s, want);
}

i128 pow2(int k) { return (i128)1 << k; }

}  // namespace

int main() {
  long cases = 0, bad = 0;
  auto done = [&](const Set& s) {
    s.print();
    cases += s.cases;
    bad += s.bad;
  };

  {  // m * 2^k + r around every rounding decision: below, at and above the tie, for even and odd m, and the carry
     // of an all-ones significand into the next binade
    Set s("designed_rounding");
    const i128 ms[] = {pow2(52), pow2(52) + 1, pow2(53) - 2, pow2(53) - 1};
    for (const i128 m : ms)
      for (int k = 1; k <= 43; ++k) {
        const i128 h = pow2(k - 1);
        const i128 rs[] = {0, 1, h - 1, h, h + 1, pow2(k) - 1};
        for (const i128 r : rs) {
          if (r < 0 || r >= pow2(k)) continue;  // (k == 1: h - 1 == 0 and h + 1 == 2^k are covered or out of range)
          check_round_both(s, m * pow2(k) + r);
        }
      }
    done(s);
  }
  {  // the exact tie alone, for m even (rounds down) and odd (rounds up) next to each other
    Set s("ties");
    const i128 base[] = {pow2(52), pow2(52) + 2, pow2(53) - 4, pow2(53) - 2};
    for (const i128 b : base)
      for (int k = 1; k <= 43; ++k) {
        check_round_both(s, b * pow2(k) + pow2(k - 1));        // even m
        check_round_both(s, (b + 1) * pow2(k) + pow2(k - 1));  // odd m
      }
    done(s);
  }
  {
    Set s("landmarks");
    const i128 v[] = {0, pow2(53) - 1, pow2(53), pow2(53) + 1, pow2(53) + 2, pow2(53) + 3, pow2(54) - 1, pow2(63) - 1,
                      pow2(63), pow2(63) + 1, pow2(64) - 1, pow2(64), pow2(64) + 1, pow2(66) + pow2(13), pow2(95) - 1,
                      pow2(95), pow2(96) - 1, pow2(126), (i128)(((u128)1 << 127) - 1)};
    for (const i128 x : v) check_round_both(s, x);
    // the int64 extremes sign-extended, as the MIN / MAX and int64 SUM call sites pass them
    const int64_t e[] = {INT64_MIN, INT64_MIN + 1, INT64_MAX, INT64_MAX - 1, INT32_MIN, INT32_MAX, -1, 1,
                         -(1ll << 53) - 1, (1ll << 53) + 1};
    for (const int64_t x : e) {
      const uint64_t got = bits_of(pa::i128_to_double(x >> 63, (uint64_t)x));
      const uint64_t want = bits_of((double)(i128)x);
      ++s.cases;
      if (got != want && ++s.bad <= 10) report(s.name, (i128)x, got, want);
    }
    check_round(s, (i128)((u128)1 << 127));  // the 128-bit minimum
    done(s);
  }
  {  // partial sums whose low part has crossed 2^32, 2^63 and 2^64 - 1, with high parts of both signs
    Set s("recombination");
    const uint64_t ls[] = {0ull, 1ull, 0xffffffffull, 1ull << 32, (1ull << 32) + 1, (1ull << 63) - 1, 1ull << 63,
                           (1ull << 63) + 1, ~0ull - 1, ~0ull, 0xffffffff00000000ull, 0x00000000ffffffffull};
    const int64_t hs[] = {0, 1, -1, 2, -2, 0x7fffffffll, 0x80000000ll, 0xffffffffll, 0x100000000ll, -0x7fffffffll,
                          -0x80000000ll, -0x80000001ll, -0xffffffffll, -0x100000000ll, -0x100000001ll,
                          (1ll << 53) + 1, -(1ll << 53) - 1, (1ll << 62), -(1ll << 62), INT64_MAX, INT64_MIN,
                          INT64_MAX - 1, INT64_MIN + 1};
    for (const int64_t h : hs)
      for (const uint64_t l : ls) check_pair(s, h, l);
    // totals that cancel: hs * 2^32 == -ls + {0, 1, -1}
    for (int k = 1; k <= 31; ++k) {
      const int64_t h = -(1ll << k);
      const uint64_t l = (uint64_t)1 << (k + 32);
      check_pair(s, h, l);
      check_pair(s, h, l + 1);
      check_pair(s, h, l - 1);
    }
    done(s);
  }
  Rng r{0x9E3779B97F4A7C15ull};
  {  // random 96-bit signed totals, as pairs (the recombination) and as integers (the rounding)
    Set s("random_pairs");
    for (int i = 0; i < 600000; ++i) {
      const int64_t h = (int64_t)r.next();
      const uint64_t l = r.next();
      check_pair(s, h, l);  // (two cases each)
    }
    done(s);
  }
  {  // random magnitudes of every bit length 1..96, both signs: uniform 96-bit values alone would all be near 2^95
    Set s("random_widths");
    for (int i = 0; i < 1000000; ++i) {
      const int len = 1 + (int)(r.next() % 96);
      u128 m = ((u128)r.next() << 64) | (u128)r.next();
      m >>= 128 - len;
      m |= (u128)1 << (len - 1);
      // half of them with a long run of zeros or ones below the significand: ties and near-ties
      const uint64_t mode = r.next() & 3;
      if (len > 54 && mode) {
        const u128 low = ((u128)1 << (len - 53)) - 1;
        const u128 halfbit = (u128)1 << (len - 54);
        if (mode == 1) m = (m & ~low) | halfbit;            // the exact tie
        else if (mode == 2) m = (m & ~low) | halfbit | 1;   // a tie and one sticky bit
        else m = (m & ~low) | (halfbit - 1);                // one below the tie
      }
      const i128 v = (i128)m;
      check_round(s, (r.next() & 1) ? -v : v);
    }
    done(s);
  }
  std::printf("TOTAL cases=%ld mismatches=%ld\n", cases, bad);
  return bad ? 1 : 0;
}
