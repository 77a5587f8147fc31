// Stand-alone check of pa::eq_any (pinot_amd/csrc/pa_eq_any.h) against a per-doc decode, for every width 1..32.
// Prints one line "nb=.. cases=.. false_neg=.. false_pos=.." per width and "TOTAL ..." at the end; exit status 1 when
// any case differs.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pa_eq_any.h"

namespace {

struct Rng {  // xorshift64*
  uint64_t s;
  uint64_t next() {
    s ^= s >> 12;
    s ^= s << 25;
    s ^= s >> 27;
    return s * 0x2545F4914F6CDD1Dull;
  }
};

uint32_t mask_of(int nb) { return nb == 32 ? 0xffffffffu : ((1u << nb) - 1u); }

// doc i of a lane: the nb bits from stream bit i*nb, word 0 first, every word MSB first
uint32_t get_doc(const std::vector<uint32_t>& w, int nb, int i) {
  uint32_t v = 0;
  for (int b = 0; b < nb; ++b) {
    const int s = i * nb + b;
    v = (v << 1) | ((w[s >> 5] >> (31 - (s & 31))) & 1u);
  }
  return v;
}

void set_doc(std::vector<uint32_t>& w, int nb, int i, uint32_t v) {
  for (int b = 0; b < nb; ++b) {
    const int s = i * nb + b;
    const uint32_t bit = 0x80000000u >> (s & 31);
    if ((v >> (nb - 1 - b)) & 1u) w[s >> 5] |= bit;
    else w[s >> 5] &= ~bit;
  }
}

template <int NB>
struct Width {
  long cases = 0, false_neg = 0, false_pos = 0;

  void check(const std::vector<uint32_t>& w, uint32_t v) {
    bool expect = false;
    for (int i = 0; i < 32; ++i) expect |= get_doc(w, NB, i) == v;
    // an exactly-sized copy, so that a read past word NB - 1 is an out-of-bounds heap read
    std::vector<uint32_t> exact(w.begin(), w.begin() + NB);
    const uint32_t* p = exact.data();
    const bool got = pa::eq_any<NB>([p](int j) { return p[j]; }, pa::eq_pattern_window(NB, v)) != 0;
    ++cases;
    if (expect && !got) ++false_neg;
    if (!expect && got) ++false_pos;
  }

  // every doc of the lane differs from v (so that only planted docs match)
  void fill_no_match(std::vector<uint32_t>& w, uint32_t v, Rng& r) {
    const uint32_t m = mask_of(NB);
    for (int i = 0; i < 32; ++i) {
      uint32_t x = (uint32_t)r.next() & m;
      if (x == v) x ^= 1u;  // (NB == 1: the other value)
      set_doc(w, NB, i, x);
    }
  }

  void run(Rng& r) {
    const uint32_t m = mask_of(NB);
    std::vector<uint32_t> w(NB);
    const uint32_t fixed[] = {0u, m, m >> 1, 1u & m};
    for (int round = 0; round < 16; ++round) {
      const uint32_t v = round < 4 ? fixed[round] : ((uint32_t)r.next() & m);
      // random lanes
      for (int k = 0; k < 8; ++k) {
        for (uint32_t& x : w) x = (uint32_t)r.next();
        check(w, v);
      }
      // no match at all; all docs equal to v
      fill_no_match(w, v, r);
      check(w, v);
      for (int i = 0; i < 32; ++i) set_doc(w, NB, i, v);
      check(w, v);
      // one match in every doc position (doc 0, doc 31 and every doc straddling a word boundary among them)
      for (int i = 0; i < 32; ++i) {
        fill_no_match(w, v, r);
        set_doc(w, NB, i, v);
        check(w, v);
      }
      // runs of 2..5 adjacent matches
      for (int len = 2; len <= 5; ++len)
        for (int i = 0; i + len <= 32; i += 3) {
          fill_no_match(w, v, r);
          for (int k = 0; k < len; ++k) set_doc(w, NB, i + k, v);
          check(w, v);
        }
      // every doc one bit off the value, then the same around one planted match
      for (int b = 0; b < NB; ++b) {
        if (NB == 1) break;  // (one bit off a 1-bit value is the only other value: covered by fill_no_match)
        for (int i = 0; i < 32; ++i) set_doc(w, NB, i, v ^ (1u << ((b + i) % NB)));
        check(w, v);
        const int at = (int)(r.next() % 32);
        set_doc(w, NB, at, v);
        check(w, v);
      }
      // v - 1 and v + 1 in every doc (borrow / carry neighbours)
      for (int i = 0; i < 32; ++i) set_doc(w, NB, i, ((i & 1) ? v + 1u : v - 1u) & m);
      if (NB > 1) check(w, v);
    }
    std::printf("nb=%d cases=%ld false_neg=%ld false_pos=%ld\n", NB, cases, false_neg, false_pos);
  }
};

long g_cases = 0, g_neg = 0, g_pos = 0;

template <int NB>
void run_all(Rng& r) {
  Width<NB> wd;
  wd.run(r);
  g_cases += wd.cases;
  g_neg += wd.false_neg;
  g_pos += wd.false_pos;
  if constexpr (NB < 32) run_all<NB + 1>(r);
}

}  // namespace

int main() {
  Rng r{0x9E3779B97F4A7C15ull};
  run_all<1>(r);
  std::printf("TOTAL cases=%ld false_neg=%ld false_pos=%ld\n", g_cases, g_neg, g_pos);
  return (g_neg || g_pos) ? 1 : 0;
}
