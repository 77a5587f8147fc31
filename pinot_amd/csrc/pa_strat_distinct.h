// Scan strategy: distinct (STRAT_DISTINCT_LDS / STRAT_DISTINCT), with what pa_distinct.hip shares with it.
// Included by pa_scan_distinct.hip and pa_distinct.hip in place of pa_scan.h, which declares the entry points it calls and includes no strategy.
#pragma once
#include "pa_scan.h"

namespace pa {

// ---------------------------------------------------------------- distinct (STRAT_DISTINCT_LDS / STRAT_DISTINCT)
// SELECT DISTINCT c1, c2, ...: the accumulator is a set of keys, one bit per key of the direct key space (bit key & 31
// of word key >> 5, DevQuery::keybits; DistinctOperator.java:55-84 offers every matching doc's record to a set). Keys
// are below 2^31 (kDistinctMaxKeys), so all key arithmetic is 32-bit.
//   STRAT_DISTINCT_LDS: a workgroup-private bitmap in LDS in front of the tile rings, zeroed in the prologue; a matching
//     doc is one no-return LDS OR; the epilogue ORs the non-zero words into the bitmap in HBM.
//   STRAT_DISTINCT: the bitmap in HBM. A plain load of the key's word comes first and the relaxed OR is issued only
//     when the bit is not yet set: a stale 0 costs a redundant atomic, and a 1 is never stale, because bits are only
//     set between two resets. Batches of 8 steps: every key of the batch, then every word load, then the atomics, so
//     one wait behind the ring's in-flight DMA (vmcnt counts in order) covers 8 loads per lane.
// In both, when every active lane of a step has its key in one word (a hot key, a key range inside one word), the
// lanes combine their bits and one of them updates (dst_combine); otherwise every lane updates on its own. Grouping the
// lanes word by word, as accumulate_step groups equal keys, was measured and dropped: with a few lanes spread over a
// few words per step it ran one ballot + shuffle pass per word and took 0.71 of 1.52 ms of the scan.
// Measurement only (tuning debug_emit, results invalid; DESIGN section 5 takes the scan apart with them): bit 0 skips the
// atomics, bit 1 also the global variant's word loads, bit 2 the in-wave combining (every lane goes on its own), bit 3
// the global variant's word load only (a plain atomic per doc: no test-before-set).
constexpr int kDstDbgNoAtomic = 1, kDstDbgNoLoad = 2, kDstDbgNoCombine = 4, kDstDbgPlainAtomic = 8;
__device__ __forceinline__ uint32_t distinct_key(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                                 const uint32_t* img, int doc_local, int64_t doc) {
  uint32_t key = 0;
  for (int j = 0; j < q->num_gb; ++j)
    key += (uint32_t)gb_component(seg->cols[q->gb_slot[j]], seg->remap[j], img, doc_local, doc) * (uint32_t)q->gb_stride[j];
  return key;
}

// One step's active lanes: true for the lanes that update the bitmap, with `bit` the OR of the bits of every lane they
// stand for: the first active lane for all of them when they share one word, else every active lane for itself.
__device__ __forceinline__ bool dst_combine(uint32_t word, uint32_t& bit, bool act, int lane) {
  const uint64_t active = __ballot(act);
  if (active == 0) return false;
  const int leader = __builtin_ctzll(active);
  const uint32_t w0 = (uint32_t)__shfl((int)word, leader);
  if (__ballot(act && word == w0) != active) return act;
  uint32_t b = act ? bit : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) b |= (uint32_t)__shfl_xor((int)b, o);
  if (lane == leader) bit = b;
  return lane == leader;
}

// The docs of one tile that passed the filter (bit i of m: the lane's doc of step i) into the bitmap.
template <int STRAT, int STEPS, int LM>
__device__ __forceinline__ void distinct_tile(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                              const uint32_t* img, int64_t doc_base, uint32_t m, int lane,
                                              unsigned char* lds) {
  auto local = [&](int i) { return LM ? 32 * lane + i : i * kWave + lane; };
  const int dbg = q->debug_emit;
  if constexpr (STRAT == STRAT_DISTINCT_LDS) {
    lds_u32_t* bm = lds_ptr(lds);
    for (int i = 0; i < STEPS; ++i) {
      const bool act = ((m >> i) & 1u) != 0;
      if (__ballot(act) == 0) continue;
      const uint32_t key = act ? distinct_key(q, seg, img, local(i), doc_base + local(i)) : 0u;
      uint32_t bit = 1u << (key & 31u);
      const bool issue = (dbg & kDstDbgNoCombine) ? act : dst_combine(key >> 5, bit, act, lane);
      if (dbg & kDstDbgNoAtomic) asm volatile("" ::"v"(bit), "v"(key));
      else if (issue) __hip_atomic_fetch_or(bm + (key >> 5), bit, WG_RLX);
    }
  } else {
    AS1 uint32_t* bm = gp(q->keybits);
    constexpr int B = 8;
    static_assert(STEPS % B == 0, "whole batches");
    for (int i0 = 0; i0 < STEPS; i0 += B) {
      const uint32_t mm = (m >> i0) & ((1u << B) - 1u);
      if (__ballot(mm != 0) == 0) continue;
      uint32_t word[B], bit[B], old[B];
      uint32_t iss = 0;
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const bool act = ((mm >> b) & 1u) != 0;
        const uint32_t key = act ? distinct_key(q, seg, img, local(i0 + b), doc_base + local(i0 + b)) : 0u;
        word[b] = key >> 5;
        bit[b] = 1u << (key & 31u);
      }
#pragma unroll
      for (int b = 0; b < B; ++b) {
        if (dbg & kDstDbgNoCombine) iss |= mm & (1u << b);
        else if (__ballot((mm >> b) & 1u) != 0 && dst_combine(word[b], bit[b], ((mm >> b) & 1u) != 0, lane)) iss |= 1u << b;
      }
#pragma unroll
      for (int b = 0; b < B; ++b)
        old[b] = !((iss >> b) & 1u) ? ~0u : ((dbg & (kDstDbgNoLoad | kDstDbgPlainAtomic)) ? 0u : bm[word[b]]);
#pragma unroll
      for (int b = 0; b < B; ++b) {
        if (dbg & kDstDbgNoAtomic) asm volatile("" ::"v"(old[b]), "v"(bit[b]), "v"(word[b]));
        else if ((bit[b] & ~old[b]) != 0) __hip_atomic_fetch_or(bm + word[b], bit[b], RLX);
      }
    }
  }
}

// STRAT_DISTINCT_LDS, start of the kernel: the workgroup's bitmap to zero.
template <int WGS>
__device__ __forceinline__ void distinct_lds_zero(const DevQuery* q, unsigned char* lds) {
  lds_u32_t* bm = lds_ptr(lds);
  const uint32_t words = (uint32_t)((q->num_keys + 31) >> 5);
  for (uint32_t w = threadIdx.x; w < words; w += WGS) bm[w] = 0u;
  __syncthreads();
}

// STRAT_DISTINCT_LDS, end of the kernel: one global OR per non-zero word.
template <int WGS>
__device__ __forceinline__ void distinct_lds_flush(const DevQuery* q, unsigned char* lds) {
  __syncthreads();
  const lds_u32_t* bm = lds_ptr(lds);
  const uint32_t words = (uint32_t)((q->num_keys + 31) >> 5);
  for (uint32_t w = threadIdx.x; w < words; w += WGS) {
    const uint32_t v = bm[w];
    if (v != 0u) __hip_atomic_fetch_or(gp(q->keybits) + w, v, RLX);
  }
}

}  // namespace pa
