// "Does any of these 32 docs equal v": the equality prefilter of the lane-major scan (scan_kernel's hoisted loop).
//
// A lane's 32 docs of an NB-bit column are the NB consecutive stream words w[0..NB): one string of 32*NB bits, word 0
// first and every word MSB first, doc i in the string's bits [i*NB, (i+1)*NB). XOR with the string "every doc equals
// v" (the pattern words) turns a matching doc into an all-zero field, and over the whole string
//     (x - L) & ~x & H  !=  0   <=>   some field of x is zero
// with L the lowest and H the highest bit of every field: the lowest zero field borrows from its own high bit, which
// ~x & H then keeps; without a zero field no field borrows, so no bit of H can go from 0 to 1. Fields above the lowest
// zero one may be flagged wrongly, which an "any" never sees. The subtraction runs from the last word to the first
// with the borrow handed on, as a field may straddle two words.
//
// Portable C++ (the host test runs the same body); on the device only the borrow step is written out, the way leaf_lm
// writes its carry: v_subb_co with the borrow in a scalar register pair.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PA_EQ_HD __host__ __device__
#else
#define PA_EQ_HD
#endif

namespace pa {

// bit b (0 = the word's MSB) of word w is stream bit 32*w + b
template <int NB>
constexpr uint32_t eq_low_bits(int w) {  // L: the last bit of every field, stream bits (i + 1)*NB - 1
  uint32_t m = 0;
  for (int i = 0; i < 32; ++i) {
    const int s = (i + 1) * NB - 1;
    if ((s >> 5) == w) m |= 0x80000000u >> (s & 31);
  }
  return m;
}
template <int NB>
constexpr uint32_t eq_high_bits(int w) {  // H: the first bit of every field, stream bits i*NB
  uint32_t m = 0;
  for (int i = 0; i < 32; ++i) {
    const int s = i * NB;
    if ((s >> 5) == w) m |= 0x80000000u >> (s & 31);
  }
  return m;
}

// The first 64 bits of v repeated every nb bits (v < 2^nb, 1 <= nb <= 32), MSB first.
PA_EQ_HD inline uint64_t eq_pattern_window(int nb, uint32_t v) {
  uint64_t w = 0;
  for (int s = 0; s < 64; s += nb) {
    const uint64_t f = (uint64_t)v << (64 - nb);  // the field at the window's top
    w |= f >> s;
  }
  return w;
}

// Pattern word j of an NB-bit column: the 32 bits of the repetition from stream bit 32*j, i.e. from bit (32*j) % NB of
// a field; (32*j) % NB + 32 <= 63, so they lie inside the window.
template <int NB>
PA_EQ_HD inline uint32_t eq_pattern_word(uint64_t window, int j) {
  return (uint32_t)((window << ((32 * j) % NB)) >> 32);
}

#if defined(__HIP_DEVICE_COMPILE__)
typedef uint64_t eq_borrow_t;  // a wave's borrow bits, one per lane (a scalar register pair)
#else
typedef uint32_t eq_borrow_t;
#endif

// Word J of the chain, then the words before it (J is a template parameter so that L and H are constants).
template <int NB, int J, class Get>
PA_EQ_HD inline void eq_any_word(Get& get, uint64_t window, eq_borrow_t& borrow, uint32_t& any) {
  constexpr uint32_t L = eq_low_bits<NB>(J), H = eq_high_bits<NB>(J);
  const uint32_t x = get(J) ^ eq_pattern_word<NB>(window, J);
  uint32_t d;
#if defined(__HIP_DEVICE_COMPILE__)
  // d = x - L - borrow, borrow out; both operands in vector registers: on gfx9 the borrow's scalar pair is the one
  // scalar operand an instruction may read, so L can be neither a literal nor a scalar register here
  asm("v_subb_co_u32_e64 %[d], %[b], %[x], %[l], %[b]" : [d] "=v"(d), [b] "+s"(borrow) : [x] "v"(x), [l] "v"(L));
#else
  const uint64_t t = (uint64_t)x - (uint64_t)L - (uint64_t)borrow;
  d = (uint32_t)t;
  borrow = (uint32_t)(t >> 32) & 1u;
#endif
  any |= d & ~x & H;
  if constexpr (J > 0) eq_any_word<NB, J - 1>(get, window, borrow, any);
}

// Non-zero iff one of the 32 fields of the words get(0) .. get(NB - 1) equals the value of the pattern `window`.
template <int NB, class Get>
PA_EQ_HD inline uint32_t eq_any(Get get, uint64_t window) {
  static_assert(NB >= 1 && NB <= 32, "dictionary ids are 1..32 bits");
  uint32_t any = 0;
  eq_borrow_t borrow = 0;
  eq_any_word<NB, NB - 1>(get, window, borrow, any);
  return any;
}

}  // namespace pa
