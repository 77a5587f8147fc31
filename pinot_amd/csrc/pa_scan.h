// Device code of the fused scan kernel (gfx950 / CDNA4 only): included by the translation units that instantiate its
// variants (pa_scan_std.hip, pa_scan_global.hip; the others through the pa_strat_*.h of their
// strategy, see "strategies in headers of their own" below), by pa_gdense.h for the helpers it shares with it, and by
// pa_kernels.hip (the other kernels).
//
// HIP kernels of the segment query hot path.
//
// One fused persistent-wave kernel per query does, for every doc of every bound segment:
//   bit-unpack the dictIds of the filter columns (FixedBitSVForwardIndexReaderV2 / PinotDataBitSet
//   semantics), evaluate the CNF filter as 64-bit wave ballots (replaces SVScanDocIdIterator /
//   BitmapBasedFilterOperator / And/Or/NotFilterOperator), build the table-wide group key
//   (DictionaryBasedGroupKeyGenerator raw key: column 0 least significant), and aggregate
//   COUNT/SUM/MIN/MAX/DISTINCTCOUNTHLL into LDS-privatised (small key spaces) or global (high
//   cardinality) accumulators (DefaultGroupByExecutor + *AggregationFunction.aggregateGroupBySV).
//
// Work decomposition: a wave owns a contiguous range of 2048-doc "wave tiles" (all segments of the
// query are concatenated); for each wave tile the forward-index words of every staged column are
// copied HBM -> LDS by LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave instruction, fully coalesced)
// into a wave-private ring of tile images, so tiles t+1 .. t+R-1 stream in while tile t is decoded. Lane l decodes
// doc 64*i + l of the tile (i = 0..31): every column of a doc lands in the same lane, and a 64-doc
// step of an nb-bit column is 2*nb consecutive LDS words (conflict-free ds_read2_b32).
#pragma once
#include <hip/hip_runtime.h>
#include "pa_device.h"
#include "pa_launch.h"
#include "pa_keys.h"
#include "pa_eq_any.h"

namespace pa {

typedef __attribute__((address_space(3))) uint32_t lds_u32_t;
// Descriptors through the constant address space: read-only during every kernel, so their fields are scalar loads the
// compiler may keep in registers across LDS atomics and stores (a generic pointer is re-read after each of them, and
// every scalar load's lgkmcnt wait also waits for the LDS operations in flight).
typedef const __attribute__((address_space(4))) struct DevSeg CSegT;
typedef const __attribute__((address_space(4))) struct DevQuery CQ;

// Every HBM access goes through address-space-1 pointers: global_* instructions instead of flat_*. A flat
// access may alias LDS, which makes the compiler put vmcnt(0) in front of later LDS reads.
#define AS1 __attribute__((address_space(1)))
template <class T>
__device__ __forceinline__ AS1 T* gp(T* p) { return (AS1 T*)p; }
template <class T>
__device__ __forceinline__ const AS1 T* gp(const T* p) { return (const AS1 T*)p; }
#define RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ void vm_wait_all() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

__device__ __forceinline__ uint32_t nbits_mask(int nb) { return nb >= 32 ? 0xffffffffu : ((1u << nb) - 1u); }

// Value of doc `doc_local` (0..2047) from a staged wave-tile region (region[-1] is a guard word).
// Stream bits [doc*nb, doc*nb+nb): the last bit e1 = doc*nb+nb-1 lies in word e1>>5; the value is the
// nb bits ending at bit position (~e1)&31 of the 64-bit window (word[we-1], word[we]).
__device__ __forceinline__ uint32_t decode_lds(const uint32_t* region, int doc_local, int nb) {
  const uint32_t e1 = (uint32_t)doc_local * (uint32_t)nb + (uint32_t)(nb - 1);
  const int we = (int)(e1 >> 5);
  const uint32_t lo = region[we];
  const uint32_t hi = region[we - 1];
  return __builtin_amdgcn_alignbit(hi, lo, (~e1) & 31u) & nbits_mask(nb);
}

// Same, straight from the HBM-resident stream (lazy columns: read only for matching docs).
__device__ __forceinline__ uint32_t decode_global(const uint32_t* words, int64_t doc, int nb) {
  const uint64_t e1 = (uint64_t)doc * (uint64_t)nb + (uint64_t)(nb - 1);
  const int64_t we = (int64_t)(e1 >> 5);
  const uint32_t lo = gp(words)[we];
  const uint32_t hi = gp(words)[we - 1];
  return __builtin_amdgcn_alignbit(hi, lo, (~(uint32_t)e1) & 31u) & nbits_mask(nb);
}

// G: the caller has no staged tile (the per-doc kernels of the numGroupsLimit path): always decode from HBM.
template <bool G = false>
__device__ __forceinline__ uint32_t decode_dict_id(const DevCol& c, const uint32_t* img, int doc_local,
                                                   int64_t doc) {
  if constexpr (G) return decode_global(c.words, doc, c.nbits);
  return c.lds_off >= 0 ? decode_lds(img + c.lds_off, doc_local, c.nbits) : decode_global(c.words, doc, c.nbits);
}

// s_waitcnt vmcnt(N) with every other counter at its maximum (gfx9 encoding: vmcnt[3:0] | vmcnt[5:4] << 14).
template <int N>
__device__ __forceinline__ void vm_wait() {
  static_assert(N >= 0 && N < 64, "vmcnt is 6 bits");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// Issue the LDS-DMA of one wave tile of every staged column of `seg` into the wave image `img`: exactly D
// wave instructions (D = the maximum over the query's segments; a segment needing fewer pads with 16-byte
// dummies into the image's guard words), so `vmcnt` counts tiles and a ring of tiles can be in flight behind
// counted waits.
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)p;
}

typedef __attribute__((address_space(3))) uint64_t lds_u64_t;
typedef __attribute__((address_space(3))) u32x4 lds_u32x4_t;
__device__ __forceinline__ lds_u32_t* lds_ptr(const void* p) { return (lds_u32_t*)(uintptr_t)lds_addr(p); }

#define WG_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP


// One LDS-DMA wave instruction (global_load_lds_dwordx4): lane l copies 16 bytes from its `src` to
// lds_base + 16*l. Issued as inline asm on purpose: the compiler's waitcnt pass cannot disambiguate LDS-DMA
// writes from later ds_reads of OTHER ring slots and would put vmcnt(0) in front of every tile's decode,
// draining the whole ring. Visibility is guaranteed by the explicit counted waits in wait_tile; vm ops the
// compiler does not know about only make its own vmcnt waits stricter, never wrong.
// NT: the load carries the `nt` cache policy (a stream read once: see stream_nt in pa_tuning.h). The modifier is part
// of the instruction text, hence a template parameter; PA_DMA16_ASM splices it into the one copy of each block.
#define PA_DMA16_ASM(MOD)                      \
  "s_mov_b32 %0, m0\n\t"                       \
  "s_mov_b32 m0, %2\n\t"                       \
  "s_nop 0\n\t"                                \
  "global_load_lds_dwordx4 %1, off" MOD "\n\t" \
  "s_mov_b32 m0, %0"
#define PA_DMA16_MASKED_ASM(MOD)               \
  "s_mov_b64 %1, exec\n\t"                     \
  "s_mov_b64 exec, %4\n\t"                     \
  "s_mov_b32 %0, m0\n\t"                       \
  "s_mov_b32 m0, %3\n\t"                       \
  "s_nop 0\n\t"                                \
  "global_load_lds_dwordx4 %2, off" MOD "\n\t" \
  "s_mov_b32 m0, %0\n\t"                       \
  "s_mov_b64 exec, %1"

template <bool NT = false>
__device__ __forceinline__ void dma16(const void* src, uint32_t lds_base) {
  uint32_t keep;
  // wave-uniform by construction; readfirstlane keeps it in an SGPR even where the compiler computed it with VALU ops
  lds_base = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_base);
  if constexpr (NT) asm volatile(PA_DMA16_ASM(" nt") : "=&s"(keep) : "v"(src), "s"(lds_base));
  else asm volatile(PA_DMA16_ASM("") : "=&s"(keep) : "v"(src), "s"(lds_base));
}

// dma16 for the lanes of `mask` only, with EXEC set and restored inside the asm block (no branch around a partial
// DMA instruction; the compiler's EXEC tracking is unaffected).
template <bool NT = false>
__device__ __forceinline__ void dma16_masked(const void* src, uint32_t lds_base, uint64_t mask) {
  uint32_t keep;
  uint64_t save;
  lds_base = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_base);
  if constexpr (NT)
    asm volatile(PA_DMA16_MASKED_ASM(" nt") : "=&s"(keep), "=&s"(save) : "v"(src), "s"(lds_base), "s"(mask));
  else
    asm volatile(PA_DMA16_MASKED_ASM("") : "=&s"(keep), "=&s"(save) : "v"(src), "s"(lds_base), "s"(mask));
}
#undef PA_DMA16_ASM
#undef PA_DMA16_MASKED_ASM

template <int STEPS>
__device__ __forceinline__ void stage_tile(const DevSeg* __restrict__ seg, int64_t wt, uint32_t* img, int lane,
                                           const int D) {
  const int ns = seg->num_staged;
  int issued = 0;
  for (int si = 0; si < ns; ++si) {
    const StageDesc& c = seg->stage[si];
    const int nb = c.nbits;
    const uint32_t* src = c.words + wt * (int64_t)(2 * STEPS * nb);  // 2*STEPS*nb stream words per wave tile
    const uint32_t dst = lds_addr(img + c.lds_off);
    const int chunks = (STEPS / 2) * nb;  // 16-byte chunks of this column's wave tile
    for (int c0 = 0; c0 < chunks; c0 += 64) {
      if (c0 + lane < chunks) dma16(src + 4 * (c0 + lane), dst + 16 * c0);
      ++issued;
    }
  }
  for (; issued < D; ++issued) {
    if (lane == 0) dma16(seg->dummy_src, lds_addr(img));
  }
}

// ---- wave reductions (all 64 lanes participate) ----
__device__ __forceinline__ int64_t wave_sum_i64(int64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ int64_t wave_min_i64(int64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const int64_t w = __shfl_xor(v, o); v = w < v ? w : v; }
  return v;
}
__device__ __forceinline__ int64_t wave_max_i64(int64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const int64_t w = __shfl_xor(v, o); v = w > v ? w : v; }
  return v;
}

// Workgroups are dispatched to the 8 XCDs round-robin (block b runs on XCD b % 8). For queries that gather per matching
// doc (dense), the scan gives block b the logical index of its place in XCD-major order, so the workgroups of one XCD
// walk one contiguous eighth of the tiles: the segments (dictionaries, remaps) an XCD touches at a time are few, and
// their lines stay in that XCD's L2 (configs[2]: HBM fetch of the emit pass 8.8 GB -> 0.9 GB per launch).
__device__ __forceinline__ int64_t xcd_major_block(int64_t b, int64_t G) {
  constexpr int kXcds = 8;
  const int64_t x = b % kXcds, j = b / kXcds, per = G / kXcds, extra = G % kXcds;
  return x * per + (x < extra ? x : extra) + j;
}

// What one wave of scan_kernel carries across its tiles, whatever the strategy. Which fields a strategy uses:
//   pair, id, astr, idm            the aggregation-only strategies (is_lane), set by lane_acc_init
//   leap_slice                     every strategy: the wave's index in logical (XCD-major) block order
//   leap_n, leap_lds               every strategy with DevQuery::leap_mode (leap_tile)
//   sel_*                          STRAT_SELECT, set by sel_state_init
// (the distinct strategies keep no per-wave state: their bitmap is the workgroup's or global)
struct WaveState {
  // Per-thread slots in LDS (the workgroup's lane-accumulator area at the front of the dynamic LDS: kLaneAccBytes per
  // thread and aggregation), so no accumulator occupies a VGPR across the tile loop: aggregation a of thread t keeps
  // (r0, r1) at pair + 16 * (a * WGS + t) and its dictId at id + 4 * (a * WGS + t) (consecutive threads 16 / 4 bytes
  // apart: conflict-free ds_read_b128 / ds_read_b32).
  uint32_t pair;   // LDS byte address of aggregation 0's (r0, r1) slot of this thread
  uint32_t id;     // LDS byte address of aggregation 0's dictId slot of this thread
  uint32_t astr;   // bytes between aggregations' pair slots (16 * WGS); dictId slots: astr / 4
  uint32_t idm;    // bit a: aggregation a's dictId was updated in the current segment run
  // fused execution statistics: this wave's slice of the E-doc list, the entries listed so far, and the LDS byte
  // address of the wave's first leap_lds_cap entries (a global store in the tile loop would make the next tile's
  // counted DMA wait longer: vmcnt counts stores too)
  uint32_t leap_slice, leap_n, leap_lds;
  // STRAT_SELECT (wave-uniform): candidates in the wave's segment of the scratch block, the wave's private bound
  // (an entry is a candidate only while it is below it), counters, the LDS byte address of the wave's select state
  uint32_t sel_n, sel_app, sel_cmp, sel_lds;
  uint64_t sel_bk, sel_br;
};

// Value an aggregation reads for one doc. For HLL returns (register << 8) | rank.
struct AggValue {
  int64_t i;
  double d;
};

template <bool G = false>
__device__ __forceinline__ AggValue agg_value(const DevAgg& A, int a, const DevSeg* __restrict__ seg,
                                              const uint32_t* img, int doc_local, int64_t doc) {
  AggValue out{0, 0.0};
  const DevCol& c = seg->cols[A.slot];
  if (c.kind == COL_SV_DICT) {
    const uint32_t id = decode_dict_id<G>(c, img, doc_local, doc);
    if (A.type == PA_AGG_DISTINCTCOUNTHLL) {
      out.i = gp(seg->hll_lut[a])[id];
    } else if (A.type == PA_AGG_DISTINCTCOUNT || A.type == PA_AGG_VALUE_HISTOGRAM) {
      out.i = seg->hll_lut[a] != nullptr ? gp(seg->hll_lut[a])[id] : id;  // table-wide value id
    } else if (A.src != SRC_DOUBLE) {
      out.i = gp(c.dict_i64)[id];
    } else {
      out.d = gp(c.dict_f64)[id];
    }
  } else {  // raw column
    int64_t iv = 0;
    double dv = 0.0;
    switch (c.vtype) {
      case PA_INT: iv = gp((const int32_t*)c.raw)[doc]; dv = (double)iv; break;
      case PA_LONG: iv = gp((const int64_t*)c.raw)[doc]; dv = (double)iv; break;
      case PA_FLOAT: { const float f = gp((const float*)c.raw)[doc]; dv = f; iv = __builtin_bit_cast(int32_t, f); } break;
      default: dv = gp((const double*)c.raw)[doc]; iv = __builtin_bit_cast(int64_t, dv); break;
    }
    if (A.type == PA_AGG_DISTINCTCOUNTHLL) {
      // MurmurHash.hash(Object): Integer/Long -> hashLong(value), Float -> hashLong(floatToRawIntBits),
      // Double -> hashLong(doubleToRawLongBits); iv already holds exactly those longs.
      out.i = hll_slot_rank(murmur_hash_long(iv), A.log2m);
    } else if (A.src != SRC_DOUBLE) {
      out.i = iv;
    } else {
      out.d = dv;
    }
  }
  return out;
}

// Register max on one byte of the u8 HLL registers in HBM (there are no byte atomics: compare-and-swap on the word
// holding it; registers only grow, so the loop ends as soon as the byte is already >= v).
__device__ __forceinline__ void atomic_max_u8(uint8_t* p, uint32_t v) {
  AS1 uint32_t* w = (AS1 uint32_t*)((uintptr_t)p & ~(uintptr_t)3);
  const uint32_t sh = ((uint32_t)(uintptr_t)p & 3u) * 8u;
  uint32_t old = __hip_atomic_load(w, RLX);
  while (((old >> sh) & 0xffu) < v) {
    const uint32_t nw = (old & ~(0xffu << sh)) | (v << sh);
    if (__hip_atomic_compare_exchange_strong(w, &old, nw, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      break;
  }
}

// ---- accumulator targets ----
template <int STRAT>
struct Acc {
  const DevQuery* q;
  unsigned char* lds;
  const PartScratch* ps;  // partitioned passes only

  __device__ __forceinline__ void add_count(int64_t key, uint32_t n) const {
    if (acc_in_lds(STRAT)) atomicAdd((uint32_t*)(lds + q->lds_count_off) + key, n);
    else __hip_atomic_fetch_add(gp(q->count) + key, (unsigned long long)n, RLX);
  }
  __device__ __forceinline__ void add_i64(const DevAgg& A, int64_t key, int64_t v) const {
    if (acc_in_lds(STRAT)) atomicAdd((unsigned long long*)(lds + A.lds_off) + key, (unsigned long long)v);
    else __hip_atomic_fetch_add(gp((unsigned long long*)A.acc_i64) + key, (unsigned long long)v, RLX);
  }
  __device__ __forceinline__ void add_f64(const DevAgg& A, int64_t key, double v) const {
    if (acc_in_lds(STRAT)) atomicAdd((double*)(lds + A.lds_off) + key, v);
    else __hip_atomic_fetch_add(gp(A.acc_f64) + key, v, RLX);
  }
  __device__ __forceinline__ void min_i64(const DevAgg& A, int64_t key, int64_t v) const {
    if (acc_in_lds(STRAT)) atomicMin((long long*)(lds + A.lds_off) + key, (long long)v);
    else __hip_atomic_fetch_min(gp((long long*)A.acc_i64) + key, (long long)v, RLX);
  }
  __device__ __forceinline__ void max_i64(const DevAgg& A, int64_t key, int64_t v) const {
    if (acc_in_lds(STRAT)) atomicMax((long long*)(lds + A.lds_off) + key, (long long)v);
    else __hip_atomic_fetch_max(gp((long long*)A.acc_i64) + key, (long long)v, RLX);
  }
  // DISTINCTCOUNT: the group saw value id v (an idempotent byte store: no atomic needed)
  __device__ __forceinline__ void set_presence(const DevAgg& A, int64_t key, int64_t v) const {
    if (acc_in_lds(STRAT)) ((uint8_t*)(lds + A.lds_off))[key * A.nvals + v] = 1;
    else gp(A.acc_hll)[key * A.nvals + v] = 1;
  }
  // VALUE_HISTOGRAM: the group aggregated value id v once more (LDS: workgroup-private u32 bins, flushed as u64 adds;
  // the planner picks LDS only when no bin can reach 2^32)
  __device__ __forceinline__ void add_hist(const DevAgg& A, int64_t key, int64_t v) const {
    if (acc_in_lds(STRAT)) atomicAdd((uint32_t*)(lds + A.lds_off) + key * A.nvals + v, 1u);
    else __hip_atomic_fetch_add(gp((unsigned long long*)A.acc_i64) + key * A.nvals + v, 1ull, RLX);
  }
  // filtered aggregations: n more docs of a lane in a group (cell = lane * num_keys + key)
  __device__ __forceinline__ void add_lane_count(int64_t cell, uint32_t n) const {
    if (acc_in_lds(STRAT)) atomicAdd((uint32_t*)(lds + q->filt->lds_lane_count_off) + cell, n);
    else __hip_atomic_fetch_add(gp(q->filt->lane_count) + cell, (unsigned long long)n, RLX);
  }
  __device__ __forceinline__ void max_hll(const DevAgg& A, int64_t key, uint32_t jr) const {
    const int64_t idx = (key << A.log2m) + (jr >> 8);
    if (acc_in_lds(STRAT)) atomicMax((uint32_t*)(lds + A.lds_off) + idx, jr & 0xffu);
    else atomic_max_u8(A.acc_hll + idx, jr & 0xffu);
  }
};

// Group-key component of one doc for group-by column j: the table-wide key id of a dictionary column (remapped), or
// the value bits of a raw column (hashed key space: INT/FLOAT 32 bits, LONG/DOUBLE 64 bits).
template <bool G = false>
__device__ __forceinline__ uint64_t gb_component(const DevCol& c, const int32_t* remap, const uint32_t* img,
                                                 int doc_local, int64_t doc) {
  if (c.kind == COL_SV_RAW) {
    switch (c.vtype) {
      case PA_INT: return (uint64_t)(uint32_t)gp((const int32_t*)c.raw)[doc];
      case PA_FLOAT: return (uint64_t)gp((const uint32_t*)c.raw)[doc];
      default: return (uint64_t)gp((const int64_t*)c.raw)[doc];
    }
  }
  uint32_t id = decode_dict_id<G>(c, img, doc_local, doc);
  if (remap != nullptr) id = (uint32_t)gp(remap)[id];
  return id;
}

// Hashed key space: the accumulator slot of a packed key (pa_keys.h: one word, or two for components wider than 64
// bits together, DevQuery::key_words; a direct key space's key is its slot). -1 if the table is full (counted as an
// overflow: the query then fails loudly at fetch).
__device__ __forceinline__ int64_t key_slot(const DevQuery* __restrict__ q, int64_t k0, int64_t k1 = 0) {
  if (!q->hashed) return k0;
  int64_t s;
  if (q->key_words == 2) {
    bool ins;
    s = ht_slot2((long long*)q->ht_keys, q->ht_mask, k0, k1, &ins);
  } else {
    s = ht_slot1((long long*)q->ht_keys, q->ht_mask, k0);
  }
  if (s < 0) __hip_atomic_fetch_add(gp(q->matched_docs) + 1, 1ull, RLX);
  return s;
}

// One aggregation's update for one set of lanes of a 64-doc step (`in`: this lane belongs to the set). grouped: the set
// shares the key k0, so SUM / MIN / MAX are reduced across the wave and lane `leader` updates once; else every lane of
// the set updates its own `key`. HLL registers, presence bytes and histogram bins are always per lane.
// (agg_apply_set: the update with the value already read — a column's by agg_update_set, an expression's by expr_step)
template <int STRAT>
__device__ __forceinline__ void agg_apply_set(const DevAgg& A, const AggValue& v, int64_t key, int64_t k0, bool in,
                                              bool grouped, int leader, int lane, const Acc<STRAT>& acc) {
  if (A.type == PA_AGG_DISTINCTCOUNTHLL) {
    if (in) acc.max_hll(A, key, (uint32_t)v.i);
  } else if (A.type == PA_AGG_DISTINCTCOUNT) {
    if (in) acc.set_presence(A, key, v.i);
  } else if (A.type == PA_AGG_VALUE_HISTOGRAM) {
    if (in) acc.add_hist(A, key, v.i);
  } else if (grouped) {
    if (A.type == PA_AGG_SUM) {
      if (A.src == SRC_INT) {
        const int64_t s = wave_sum_i64(in ? v.i : 0);
        if (lane == leader) acc.add_i64(A, k0, s);
      } else if (A.src == SRC_LONG) {
        const int64_t lo = wave_sum_i64(in ? (int64_t)(uint32_t)v.i : 0);
        const int64_t hi = wave_sum_i64(in ? (v.i >> 32) : 0);
        if (lane == leader) {
          acc.add_i64(A, 2 * k0, lo);
          acc.add_i64(A, 2 * k0 + 1, hi);
        }
      } else {
        const double s = wave_sum_f64(in ? v.d : 0.0);
        if (lane == leader) acc.add_f64(A, k0, s);
      }
    } else {
      const int64_t e = A.src != SRC_DOUBLE ? v.i : f64_order_encode(v.d);
      if (A.type == PA_AGG_MIN) {
        const int64_t r = wave_min_i64(in ? e : INT64_MAX);
        if (lane == leader) acc.min_i64(A, k0, r);
      } else {
        const int64_t r = wave_max_i64(in ? e : INT64_MIN);
        if (lane == leader) acc.max_i64(A, k0, r);
      }
    }
  } else if (in) {
    if (A.type == PA_AGG_SUM) {
      if (A.src == SRC_INT) {
        acc.add_i64(A, key, v.i);
      } else if (A.src == SRC_LONG) {
        acc.add_i64(A, 2 * key, (int64_t)(uint32_t)v.i);
        acc.add_i64(A, 2 * key + 1, v.i >> 32);
      } else {
        acc.add_f64(A, key, v.d);
      }
    } else {
      const int64_t e = A.src != SRC_DOUBLE ? v.i : f64_order_encode(v.d);
      if (A.type == PA_AGG_MIN) acc.min_i64(A, key, e);
      else acc.max_i64(A, key, e);
    }
  }
}

template <int STRAT>
__device__ __forceinline__ void agg_update_set(const DevAgg& A, int a, const DevSeg* __restrict__ seg,
                                               const uint32_t* img, int doc_local, int64_t doc, int64_t key, int64_t k0,
                                               bool in, bool grouped, int leader, int lane, const Acc<STRAT>& acc) {
  AggValue v{0, 0.0};
  if (in) v = agg_value(A, a, seg, img, doc_local, doc);
  agg_apply_set<STRAT>(A, v, key, k0, in, grouped, leader, lane, acc);
}

// (masks over values, not conditionals between array elements: the compiler turns a chain of conditional element reads
// back into one indexed load, and the array would then live in scratch memory; cf. filt_pair_mask)
__device__ __forceinline__ uint64_t expr_get(const uint64_t (&v)[PA_MAX_EXPR_REGS], int i) {
  uint64_t r = 0;
#pragma unroll
  for (int k = 0; k < PA_MAX_EXPR_REGS; ++k) r |= v[k] & (0ull - (uint64_t)(i == k));
  return r;
}
__device__ __forceinline__ void expr_set(uint64_t (&v)[PA_MAX_EXPR_REGS], int i, uint64_t x) {
#pragma unroll
  for (int k = 0; k < PA_MAX_EXPR_REGS; ++k) {
    const uint64_t m = 0ull - (uint64_t)(i == k);
    v[k] = (x & m) | (v[k] & ~m);
  }
}
// What expr_step hands accumulate_step (pa_strat_expr.h "expressions"): the programs' descriptor and their results for this
// lane's doc.
struct ExprVals {
  const ExprDesc* E;
  uint64_t res[PA_MAX_EXPRS];
};

// Accumulate the matched lanes (`matched` = wave mask) of one 64-doc step. The expression strategies pass `ev`: a
// group-by position or aggregation with a program takes that program's result in place of its column's value.
template <int STRAT>
__device__ __forceinline__ void accumulate_step(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                                const uint32_t* img, int doc_local, int64_t doc,
                                                uint64_t matched, int lane, const Acc<STRAT>& acc,
                                                const ExprVals* ev = nullptr) {
  bool mine = (matched >> lane) & 1ull;
  // table-wide group key (DictionaryBasedGroupKeyGenerator: rawKey = sum dictId_j * prod_{k<j} card_k), or the packed
  // key's accumulator slot in the hashed key space
  int64_t key = 0;
  if (mine) {
    int64_t kw[2] = {0, 0};  // (two words: DevQuery::gb_word)
    if constexpr (is_expr(STRAT)) {
      for (int j = 0; j < q->num_gb; ++j) {
        const int ge = ev->E->gb_expr[j];
        const uint64_t comp = ge >= 0 ? expr_get(ev->res, ge)
                                      : gb_component(seg->cols[q->gb_slot[j]], seg->remap[j], img, doc_local, doc);
        kw[q->gb_word[j]] += (int64_t)(comp * (uint64_t)q->gb_stride[j]);
      }
    } else {
      for (int j = 0; j < q->num_gb; ++j)
        kw[q->gb_word[j]] += (int64_t)(gb_component(seg->cols[q->gb_slot[j]], seg->remap[j], img, doc_local, doc) *
                                       (uint64_t)q->gb_stride[j]);
    }
    key = key_slot(q, kw[0], kw[1]);
    if (key < 0) mine = false;
  }
  matched &= __ballot(mine);

  uint64_t pending = matched;
  bool first = true;
  while (pending) {
    // Pick the group of lanes sharing the first pending lane's key; if that group is small on the first
    // pass (high-cardinality keys) give up on grouping and let every pending lane update on its own.
    const int leader = __builtin_ctzll(pending);
    const int64_t k0 = __shfl(key, leader);
    const uint64_t same = __ballot(key == k0) & pending;
    const bool grouped = !first || (__builtin_popcountll(same) * 4 >= __builtin_popcountll(pending));
    first = false;
    const uint64_t set = grouped ? same : pending;
    pending &= ~set;
    const bool in = (set >> lane) & 1ull;

    if (grouped) {
      if (lane == leader) acc.add_count(k0, (uint32_t)__builtin_popcountll(set));
    } else if (in) {
      acc.add_count(key, 1u);
    }
    for (int a = 0; a < q->num_aggs; ++a) {
      const DevAgg& A = q->aggs[a];
      if (A.type == PA_AGG_COUNT) continue;
      if constexpr (is_expr(STRAT)) {
        const int ae = ev->E->agg_expr[a];
        if (ae >= 0) {  // the program's value: a double as SRC_DOUBLE, an int64 as SRC_LONG
          const uint64_t x = expr_get(ev->res, ae);
          const AggValue v{(int64_t)x, __builtin_bit_cast(double, x)};
          agg_apply_set<STRAT>(A, v, key, k0, in, grouped, leader, lane, acc);
          continue;
        }
      }
      agg_update_set<STRAT>(A, a, seg, img, doc_local, doc, key, k0, in, grouped, leader, lane, acc);
    }
  }
}

// Value of an aggregation at value index `vi` of an MV dictionary column (SUMMV / MINMV / MAXMV / DISTINCTCOUNTHLLMV).
__device__ __forceinline__ AggValue agg_value_mv(const DevAgg& A, int a, const DevSeg* __restrict__ seg,
                                                 const DevCol& c, int64_t vi) {
  AggValue out{0, 0.0};
  const uint32_t id = decode_global(c.words, vi, c.nbits);
  if (A.type == PA_AGG_DISTINCTCOUNTHLL) out.i = gp(seg->hll_lut[a])[id];
  else if (A.type == PA_AGG_DISTINCTCOUNT || A.type == PA_AGG_VALUE_HISTOGRAM)
    out.i = seg->hll_lut[a] != nullptr ? gp(seg->hll_lut[a])[id] : id;
  else if (A.src != SRC_DOUBLE) out.i = gp(c.dict_i64)[id];
  else out.d = gp(c.dict_f64)[id];
  return out;
}

template <int STRAT>
__device__ __forceinline__ void update_one(const DevAgg& A, int64_t key, const AggValue& v, const Acc<STRAT>& acc) {
  if (A.type == PA_AGG_DISTINCTCOUNTHLL) {
    acc.max_hll(A, key, (uint32_t)v.i);
  } else if (A.type == PA_AGG_DISTINCTCOUNT) {
    acc.set_presence(A, key, v.i);
  } else if (A.type == PA_AGG_VALUE_HISTOGRAM) {
    acc.add_hist(A, key, v.i);
  } else if (A.type == PA_AGG_SUM) {
    if (A.src == SRC_INT) {
      acc.add_i64(A, key, v.i);
    } else if (A.src == SRC_LONG) {
      acc.add_i64(A, 2 * key, (int64_t)(uint32_t)v.i);
      acc.add_i64(A, 2 * key + 1, v.i >> 32);
    } else {
      acc.add_f64(A, key, v.d);
    }
  } else {
    const int64_t e = A.src != SRC_DOUBLE ? v.i : f64_order_encode(v.d);
    if (A.type == PA_AGG_MIN) acc.min_i64(A, key, e);
    else acc.max_i64(A, key, e);
  }
}

// One aggregation update of group `key` in the workgroup's LDS accumulators (STRAT_LDS layout: DevAgg::lds_off), through
// address-space-3 pointers (ds_* atomics). v: AggValue of agg_value (HLL: register << 8 | rank; DISTINCTCOUNT and
// VALUE_HISTOGRAM: value id).
__device__ __forceinline__ void lds_update(int type, int src, int log2m, int64_t nvals, uint32_t off,
                                           unsigned char* lds, int64_t key, const AggValue& v) {
  unsigned char* b = lds + off;
  switch (type) {
    case PA_AGG_SUM:
      if (src == SRC_INT) {
        __hip_atomic_fetch_add((lds_u64_t*)lds_ptr(b) + key, (uint64_t)v.i, WG_RLX);
      } else if (src == SRC_LONG) {
        __hip_atomic_fetch_add((lds_u64_t*)lds_ptr(b) + 2 * key, (uint64_t)(uint32_t)v.i, WG_RLX);
        __hip_atomic_fetch_add((lds_u64_t*)lds_ptr(b) + 2 * key + 1, (uint64_t)(v.i >> 32), WG_RLX);
      } else {
        __hip_atomic_fetch_add((__attribute__((address_space(3))) double*)lds_ptr(b) + key, v.d, WG_RLX);
      }
      break;
    case PA_AGG_COUNT_MV:
      __hip_atomic_fetch_add((lds_u64_t*)lds_ptr(b) + key, (uint64_t)v.i, WG_RLX);
      break;
    case PA_AGG_MIN:
    case PA_AGG_MAX: {
      const int64_t e = src != SRC_DOUBLE ? v.i : f64_order_encode(v.d);
      __attribute__((address_space(3))) int64_t* t = (__attribute__((address_space(3))) int64_t*)lds_ptr(b) + key;
      if (type == PA_AGG_MIN) __hip_atomic_fetch_min(t, e, WG_RLX);
      else __hip_atomic_fetch_max(t, e, WG_RLX);
    } break;
    case PA_AGG_DISTINCTCOUNTHLL:
      __hip_atomic_fetch_max(lds_ptr(b) + ((key << log2m) + ((uint32_t)v.i >> 8)), (uint32_t)v.i & 0xffu, WG_RLX);
      break;
    case PA_AGG_DISTINCTCOUNT:
      ((__attribute__((address_space(3))) uint8_t*)lds_ptr(b))[key * nvals + v.i] = 1;
      break;
    case PA_AGG_VALUE_HISTOGRAM:
      __hip_atomic_fetch_add(lds_ptr(b) + (key * nvals + v.i), 1u, WG_RLX);
      break;
    default: break;
  }
}

// LDS-privatised accumulators, lane-major tile: each lane walks its own matching docs (doc 32 * lane + i), four per
// batch — every group-by decode of the batch, then every remap gather, then every aggregation value load, then the LDS
// updates — so a tile costs the wave max-popcount / 4 dependent round trips instead of one per 64-doc step (the
// step-major path waits on each step's value loads before its wave-level key grouping). Lanes sharing a key meet in
// the LDS atomics (DefaultGroupByExecutor.aggregateGroupBySV per doc).
template <int kB>
__device__ __forceinline__ void accumulate_lds_lm(const DevQuery* __restrict__ q_in, const DevSeg* __restrict__ seg,
                                                  const uint32_t* img, int64_t doc_base, uint32_t m, int lane,
                                                  unsigned char* lds) {
  CQ* q = (CQ*)(uintptr_t)q_in;
  CSegT* cs = (CSegT*)(uintptr_t)seg;
  const int64_t d0 = doc_base + 32 * lane;
  lds_u32_t* cnt = lds_ptr(lds + q->lds_count_off);
  const int ngb = q->num_gb, na = q->num_aggs;
  while (__ballot(m != 0) != 0) {
    bool on[kB];
    int il[kB];
#pragma unroll
    for (int k = 0; k < kB; ++k) {
      on[k] = m != 0;
      il[k] = on[k] ? __builtin_ctz(m) : 0;
      m &= m - 1u;
    }
    int64_t key[kB];
#pragma unroll
    for (int k = 0; k < kB; ++k) key[k] = 0;
    for (int j = 0; j < ngb; ++j) {
      const int slot = q->gb_slot[j];
      const int gl = cs->cols[slot].lds_off, gn = cs->cols[slot].nbits;
      const uint32_t* gw = cs->cols[slot].words;
      const int32_t* rm = cs->remap[j];
      const int64_t st = q->gb_stride[j];
      uint32_t id[kB];
#pragma unroll
      for (int k = 0; k < kB; ++k) {
        id[k] = 0u;
        if (on[k]) id[k] = gl >= 0 ? decode_lds(img + gl, 32 * lane + il[k], gn) : decode_global(gw, d0 + il[k], gn);
      }
      if (rm != nullptr) {
#pragma unroll
        for (int k = 0; k < kB; ++k)
          if (on[k]) id[k] = (uint32_t)gp(rm)[id[k]];
      }
#pragma unroll
      for (int k = 0; k < kB; ++k) key[k] += (int64_t)id[k] * st;
    }
#pragma unroll
    for (int k = 0; k < kB; ++k)
      if (on[k]) __hip_atomic_fetch_add(cnt + key[k], 1u, WG_RLX);
    for (int a = 0; a < na; ++a) {
      const int type = q->aggs[a].type;
      if (type == PA_AGG_COUNT) continue;
      const DevAgg& A = q_in->aggs[a];
      AggValue v[kB];
#pragma unroll
      for (int k = 0; k < kB; ++k)
        v[k] = on[k] ? agg_value(A, a, seg, img, 32 * lane + il[k], d0 + il[k]) : AggValue{0, 0.0};
      const int src = q->aggs[a].src, lg = q->aggs[a].log2m;
      const int64_t nv = q->aggs[a].nvals;
      const uint32_t off = (uint32_t)q->aggs[a].lds_off;
#pragma unroll
      for (int k = 0; k < kB; ++k)
        if (on[k]) lds_update(type, src, lg, nv, off, lds, key[k], v[k]);
    }
  }
}

// accumulate_lds_lm for a dense lane-major tile whose non-COUNT aggregations (SUM / MIN / MAX) all read one raw column
// (slot q->lds_raw_slot): that column's values of the tile arrive as coalesced 16-byte loads (instruction k, lane l:
// docs VPL * (64 k + l) + j, as in lane_raw_dense) with their match bits from the lanes owning the docs (ds_bpermute);
// the lane decodes the group key of each such doc from the staged image (any doc of the tile is in it) and updates.
template <int VB>
__device__ __forceinline__ void accumulate_lds_raw_dense(const DevQuery* __restrict__ q_in,
                                                         const DevSeg* __restrict__ seg, const uint32_t* img,
                                                         int64_t doc_base, uint32_t m, int lane, unsigned char* lds) {
  CQ* q = (CQ*)(uintptr_t)q_in;
  CSegT* cs = (CSegT*)(uintptr_t)seg;
  constexpr int VPL = 16 / VB;
  constexpr int NI = 2048 * VB / 1024;
  constexpr int KB = VB == 8 ? 4 : 8;  // loads in flight per batch (16 VGPRs of values)
  const int rs = q->lds_raw_slot;
  const int vt = cs->cols[rs].vtype;
  const AS1 u32x4* p = (const AS1 u32x4*)((const char*)cs->cols[rs].raw + doc_base * VB) + lane;
  lds_u32_t* cnt = lds_ptr(lds + q->lds_count_off);
  const int ngb = q->num_gb, na = q->num_aggs;
#pragma unroll 1
  for (int k0 = 0; k0 < NI; k0 += KB) {
    u32x4 w[KB];
    uint32_t mb[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      w[k] = p[(k0 + k) * kWave];
      const int owner = 2 * VPL * (k0 + k) + ((VPL * lane) >> 5);
      mb[k] = ((uint32_t)__builtin_amdgcn_ds_bpermute(owner << 2, (int)m) >> ((VPL * lane) & 31)) & ((1u << VPL) - 1u);
    }
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      const int k1 = k0 + k;
      int64_t key[VPL];
#pragma unroll
      for (int j = 0; j < VPL; ++j) key[j] = 0;
      for (int g = 0; g < ngb; ++g) {
        const int slot = q->gb_slot[g];
        const int gl = cs->cols[slot].lds_off, gn = cs->cols[slot].nbits;
        const uint32_t* gw = cs->cols[slot].words;
        const int32_t* rm = cs->remap[g];
        const int64_t st = q->gb_stride[g];
        uint32_t id[VPL];
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
          const int dl = VPL * (64 * k1 + lane) + j;  // tile-local doc (lane-major image: any doc is decodable here)
          id[j] = 0u;
          if ((mb[k] >> j) & 1u) id[j] = gl >= 0 ? decode_lds(img + gl, dl, gn) : decode_global(gw, doc_base + dl, gn);
        }
        if (rm != nullptr) {
#pragma unroll
          for (int j = 0; j < VPL; ++j)
            if ((mb[k] >> j) & 1u) id[j] = (uint32_t)gp(rm)[id[j]];
        }
#pragma unroll
        for (int j = 0; j < VPL; ++j) key[j] += (int64_t)id[j] * st;
      }
#pragma unroll
      for (int j = 0; j < VPL; ++j) {
        if (!((mb[k] >> j) & 1u)) continue;
        const uint64_t x = VB == 8 ? ((uint64_t)w[k][2 * j + 1] << 32) | w[k][2 * j] : (uint64_t)w[k][j];
        AggValue v;
        if (vt == PA_INT) { v.i = (int64_t)(int32_t)(uint32_t)x; v.d = (double)v.i; }
        else if (vt == PA_LONG) { v.i = (int64_t)x; v.d = (double)v.i; }
        else if (vt == PA_FLOAT) { v.d = __builtin_bit_cast(float, (uint32_t)x); v.i = (int64_t)(int32_t)(uint32_t)x; }
        else { v.d = __builtin_bit_cast(double, x); v.i = (int64_t)x; }
        __hip_atomic_fetch_add(cnt + key[j], 1u, WG_RLX);
        for (int a = 0; a < na; ++a) {
          const int type = q->aggs[a].type;
          if (type == PA_AGG_COUNT) continue;
          lds_update(type, q->aggs[a].src, 0, 0, (uint32_t)q->aggs[a].lds_off, lds, key[j], v);
        }
      }
    }
  }
}

// COUNT += 1 and every aggregation of one doc into accumulator slot `key`; an MV aggregation column contributes every
// value of the doc (aggregateGroupByMV / *MVAggregationFunction).
template <int STRAT, bool G = false>
__device__ __forceinline__ void update_doc_key(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                               const uint32_t* img, int doc_local, int64_t doc, int64_t key,
                                               const Acc<STRAT>& acc) {
  acc.add_count(key, 1u);
  for (int a = 0; a < q->num_aggs; ++a) {
    const DevAgg& A = q->aggs[a];
    if (A.type == PA_AGG_COUNT) continue;
    const DevCol& c = seg->cols[A.slot];
    if (c.kind == COL_MV_DICT) {
      const int32_t v0 = gp(c.mv_off)[doc], v1 = gp(c.mv_off)[doc + 1];
      if (A.type == PA_AGG_COUNT_MV) {
        acc.add_i64(A, key, (int64_t)(v1 - v0));
        continue;
      }
      for (int32_t vi = v0; vi < v1; ++vi) update_one<STRAT>(A, key, agg_value_mv(A, a, seg, c, vi), acc);
    } else {
      update_one<STRAT>(A, key, agg_value<G>(A, a, seg, img, doc_local, doc), acc);
    }
  }
}

// One matching doc of a query with a multi-value group-by or aggregation column, on its own lane (no wave
// grouping): the doc expands into the cartesian product of its MV group-by values (DictionaryBasedGroupKeyGenerator
// .getIntRawKeys; duplicates included, like the reference), and every key receives COUNT += 1 and every aggregation
// — over all values of an MV aggregation column (aggregateGroupByMV / *MVAggregationFunction).
template <int STRAT>
__device__ void accumulate_doc_mv(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                  const uint32_t* img, int doc_local, int64_t doc, const Acc<STRAT>& acc) {
  int64_t base_key[2] = {0, 0};
  int nmv = 0;
  int mv_gb[PA_MAX_GROUP_BY];
  int32_t mv_s[PA_MAX_GROUP_BY], mv_n[PA_MAX_GROUP_BY];
  int64_t combos = 1;
  for (int j = 0; j < q->num_gb; ++j) {
    const DevCol& c = seg->cols[q->gb_slot[j]];
    if (c.kind == COL_MV_DICT) {
      const int32_t s0 = gp(c.mv_off)[doc];
      mv_gb[nmv] = j;
      mv_s[nmv] = s0;
      mv_n[nmv] = gp(c.mv_off)[doc + 1] - s0;
      combos *= mv_n[nmv];
      ++nmv;
    } else {
      base_key[q->gb_word[j]] += (int64_t)(gb_component(c, seg->remap[j], img, doc_local, doc) * (uint64_t)q->gb_stride[j]);
    }
  }
  for (int64_t cb = 0; cb < combos; ++cb) {
    int64_t kw[2] = {base_key[0], base_key[1]};
    int64_t rem = cb;
    for (int t = 0; t < nmv; ++t) {
      const int j = mv_gb[t];
      const DevCol& c = seg->cols[q->gb_slot[j]];
      const int64_t digit = rem % mv_n[t];
      rem /= mv_n[t];
      uint32_t id = decode_global(c.words, mv_s[t] + digit, c.nbits);
      const int32_t* rm = seg->remap[j];
      if (rm != nullptr) id = (uint32_t)gp(rm)[id];
      kw[q->gb_word[j]] += (int64_t)id * q->gb_stride[j];
    }
    const int64_t key = key_slot(q, kw[0], kw[1]);
    if (key < 0) continue;
    // numGroupsLimit, walk form (direct key space): only the keys the segment admitted
    if (seg->admit != nullptr && !((gp(seg->admit)[key >> 5] >> (key & 31)) & 1u)) continue;
    update_doc_key<STRAT>(q, seg, img, doc_local, doc, key, acc);
  }
}

// scan_kernel's prologue and epilogue of each strategy are functions next to that strategy's code (here: STRAT_LDS).
// Their pointer parameters carry no __restrict__: the qualifier on an inlined helper gives its body alias scopes of
// its own, and the kernels then compile differently.
// STRAT_LDS, start of the kernel: the workgroup's LDS accumulators to their identities.
template <int WGS>
__device__ __forceinline__ void lds_acc_zero(const DevQuery* q, unsigned char* lds_acc) {
  const int64_t K = q->num_keys;
  uint32_t* cnt = (uint32_t*)(lds_acc + q->lds_count_off);
  for (int64_t k = threadIdx.x; k < K; k += WGS) cnt[k] = 0;
  for (int a = 0; a < q->num_aggs; ++a) {
    const DevAgg& A = q->aggs[a];
    if (A.type == PA_AGG_COUNT) continue;
    if (A.type == PA_AGG_DISTINCTCOUNTHLL) {
      uint32_t* r = (uint32_t*)(lds_acc + A.lds_off);
      for (int64_t k = threadIdx.x; k < (K << A.log2m); k += WGS) r[k] = 0;
    } else if (A.type == PA_AGG_DISTINCTCOUNT) {
      uint32_t* r = (uint32_t*)(lds_acc + A.lds_off);
      for (int64_t k = threadIdx.x; k < K * A.nvals / 4; k += WGS) r[k] = 0;
    } else if (A.type == PA_AGG_VALUE_HISTOGRAM) {
      uint32_t* r = (uint32_t*)(lds_acc + A.lds_off);
      for (int64_t k = threadIdx.x; k < K * A.nvals; k += WGS) r[k] = 0;
    } else {
      int64_t* r = (int64_t*)(lds_acc + A.lds_off);
      const int64_t init = A.type == PA_AGG_MIN ? INT64_MAX : (A.type == PA_AGG_MAX ? INT64_MIN : 0);  // SUM, COUNT_MV: 0
      const int64_t n = (A.type == PA_AGG_SUM && A.src == SRC_LONG) ? 2 * K : K;
      for (int64_t k = threadIdx.x; k < n; k += WGS) r[k] = init;  // SUM(double) 0.0 == all-zero bits
    }
  }
  __syncthreads();
}

// Key k of one aggregation's workgroup-private LDS accumulators into the global ones (VALUE_HISTOGRAM bins leave in
// lds_acc_flush's own loop).
__device__ __forceinline__ void lds_flush_agg(const DevAgg& A, int64_t k, unsigned char* lds_acc) {
  switch (A.type) {
    case PA_AGG_SUM:
      if (A.src == SRC_INT) {
        __hip_atomic_fetch_add(gp((unsigned long long*)A.acc_i64) + k, ((const unsigned long long*)(lds_acc + A.lds_off))[k], RLX);
      } else if (A.src == SRC_LONG) {
        const unsigned long long* r = (const unsigned long long*)(lds_acc + A.lds_off);
        __hip_atomic_fetch_add(gp((unsigned long long*)A.acc_i64) + 2 * k, r[2 * k], RLX);
        __hip_atomic_fetch_add(gp((unsigned long long*)A.acc_i64) + 2 * k + 1, r[2 * k + 1], RLX);
      } else {
        __hip_atomic_fetch_add(gp(A.acc_f64) + k, ((const double*)(lds_acc + A.lds_off))[k], RLX);
      }
      break;
    case PA_AGG_COUNT_MV:
      __hip_atomic_fetch_add(gp((unsigned long long*)A.acc_i64) + k, ((const unsigned long long*)(lds_acc + A.lds_off))[k], RLX);
      break;
    case PA_AGG_MIN: __hip_atomic_fetch_min(gp((long long*)A.acc_i64) + k, ((const long long*)(lds_acc + A.lds_off))[k], RLX); break;
    case PA_AGG_MAX: __hip_atomic_fetch_max(gp((long long*)A.acc_i64) + k, ((const long long*)(lds_acc + A.lds_off))[k], RLX); break;
    case PA_AGG_DISTINCTCOUNT: {  // presence words with a value seen here -> bytes of the global block
      const uint32_t* r = (const uint32_t*)(lds_acc + A.lds_off + k * A.nvals);
      AS1 uint8_t* g = gp(A.acc_hll) + k * A.nvals;
      for (int64_t j = 0; j < A.nvals / 4; ++j) {
        const uint32_t w = r[j];
        if (w == 0) continue;
        for (int b = 0; b < 4; ++b)
          if ((w >> (8 * b)) & 0xffu) g[4 * j + b] = 1;
      }
    } break;
    case PA_AGG_DISTINCTCOUNTHLL: {
      const uint32_t* r = (const uint32_t*)(lds_acc + A.lds_off) + (k << A.log2m);
      uint8_t* g = A.acc_hll + (k << A.log2m);
      for (int j = 0; j < (1 << A.log2m); ++j)
        if (r[j] != 0) atomic_max_u8(g + j, r[j]);
    } break;
    default: break;
  }
}

// STRAT_LDS, end of the kernel: every key the workgroup saw into the global accumulators.
template <int WGS>
__device__ __forceinline__ void lds_acc_flush(const DevQuery* q, unsigned char* lds_acc) {
  __syncthreads();
  const int64_t K = q->num_keys;
  const uint32_t* cnt = (const uint32_t*)(lds_acc + q->lds_count_off);
  for (int64_t k = threadIdx.x; k < K; k += WGS) {
    const uint32_t c = cnt[k];
    if (c == 0) continue;
    __hip_atomic_fetch_add(gp(q->count) + k, (unsigned long long)c, RLX);
    for (int a = 0; a < q->num_aggs; ++a) lds_flush_agg(q->aggs[a], k, lds_acc);
  }
  // VALUE_HISTOGRAM: a row can hold tens of thousands of bins, so the workgroup's threads walk the bins of all keys
  // (not one thread per key): every non-zero u32 bin becomes one u64 add into the global block
  for (int a = 0; a < q->num_aggs; ++a) {
    const DevAgg& A = q->aggs[a];
    if (A.type != PA_AGG_VALUE_HISTOGRAM) continue;
    const uint32_t* r = (const uint32_t*)(lds_acc + A.lds_off);
    AS1 unsigned long long* g = gp((unsigned long long*)A.acc_i64);
    for (int64_t i = threadIdx.x; i < K * A.nvals; i += WGS)
      if (r[i] != 0) __hip_atomic_fetch_add(g + i, (unsigned long long)r[i], RLX);
  }
}

// RAW_SET membership (RawValueBasedInPredicateEvaluatorFactory's value sets): the set's first / last value bound it,
// then a binary search of the sorted values (a few L2-resident loads per doc)
template <class LeafT>
__device__ __forceinline__ bool raw_set_has(const LeafT& L, int64_t x) {
  if (x < L.ilo || x > L.ihi) return false;
  const AS1 int64_t* v = gp((const int64_t*)L.lut);
  int32_t b = 0, n = L.span;
  while (n > 1) {
    const int32_t h = n >> 1;
    b = v[b + h] <= x ? b + h : b;
    n -= h;
  }
  return v[b] == x;
}
template <class LeafT>
__device__ __forceinline__ bool raw_set_has(const LeafT& L, double x) {
  if (!(x >= L.dlo && x <= L.dhi)) return false;
  const AS1 double* v = gp((const double*)L.lut);
  int32_t b = 0, n = L.span;
  while (n > 1) {
    const int32_t h = n >> 1;
    b = v[b + h] <= x ? b + h : b;
    n -= h;
  }
  return v[b] == x;
}

// Match word of one leaf over a whole wave tile: bit i of lane l <=> doc 64*i + l of the tile matches.
// Leaf parameters are loaded once per tile; the 32 decodes are independent, so the LDS reads pipeline.
template <int STEPS, class LeafT = DevLeaf>
__device__ __forceinline__ uint32_t leaf_bits(const LeafT& L, const uint32_t* img, int64_t doc_base, int lane) {
  uint32_t bits = 0;
  if (L.kind == PA_LEAF_DICT_RANGE || L.kind == PA_LEAF_DICT_SET) {
    const int nb = L.nbits;
    const uint32_t mask = nbits_mask(nb);
    const uint32_t e1 = (uint32_t)lane * (uint32_t)nb + (uint32_t)(nb - 1);
    const uint32_t sh = (~e1) & 31u;
    const int step = 2 * nb;  // stream words per 64-doc step
    {
      const uint32_t* p = img + L.lds_off + (int)(e1 >> 5);
      if (L.kind == PA_LEAF_DICT_RANGE) {
        // MSB-aligned decode: the window starts at the word holding the value's first bit (or the word before,
        // when that bit is bit 0 of a word), so t = alignbit(.) carries the value in its top nb bits with junk
        // below. With lo' = lo << (32-nb) and hi' = span << (32-nb) - 1 (host-side),
        //   lo <= v < lo + span  <=>  (t - lo') <= hi'   (unsigned; exact for any junk bits).
        // Non-matches accumulate as nm = 2*nm + borrow(hi' - (t - lo')): sub, sub_co, addc per 64 docs.
        const uint32_t lo_t = (uint32_t)L.lo, hi_t = (uint32_t)L.span;  // pre-shifted by the host
        const uint32_t b0 = (uint32_t)lane * (uint32_t)nb;
        const uint32_t o = b0 & 31u;
        const int ws = (int)(b0 >> 5) - (o == 0 ? 1 : 0);
        const uint32_t shr = (32u - o) & 31u;
        // every scalar parameter in SGPRs before the first LDS read: a scalar load between LDS reads forces
        // lgkmcnt(0) (SMEM returns out of order) and serialises the reads. The window pointer goes through the asm
        // as a 32-bit LDS offset and comes back as an address-space-3 pointer (ds_read; a generic pointer rebuilt
        // from 32 bits would lose the shared aperture and address global memory).
        uint32_t pw_off = lds_addr(img + L.lds_off + ws);
        asm volatile("" : "+v"(pw_off) : "s"(lo_t), "s"(hi_t), "s"(step));
        const lds_u32_t* pw = (const lds_u32_t*)(uintptr_t)pw_off;
        uint32_t w0[STEPS], w1[STEPS];
#pragma unroll
        for (int i = 0; i < STEPS; ++i) {
          w0[i] = pw[i * step];
          w1[i] = pw[i * step + 1];
        }
        uint32_t nm = 0;
#pragma unroll
        for (int i = STEPS - 1; i >= 0; --i) {
          const uint32_t t = __builtin_amdgcn_alignbit(w0[i], w1[i], shr);
          uint32_t u;
          // u = t - lo'; borrow = hi' < u (non-match); nm = 2*nm + borrow  (the compiler otherwise rewrites the
          // carry-add into cndmask + or)
          asm("v_sub_u32_e64 %[u], %[t], %[lo]\n\t"
              "v_sub_co_u32_e32 %[u], vcc, %[hi], %[u]\n\t"
              "v_addc_co_u32_e32 %[nm], vcc, %[nm], %[nm], vcc"
              : [nm] "+v"(nm), [u] "=&v"(u)
              : [t] "v"(t), [lo] "s"(lo_t), [hi] "s"(hi_t)
              : "vcc");
        }
        bits = STEPS == 32 ? ~nm : (~nm & ((1u << STEPS) - 1u));
        (void)mask;
        (void)p;
      } else {
        const AS1 uint32_t* lut = gp(L.lut);
#pragma unroll 8
        for (int i = 0; i < STEPS; ++i) {
          const uint32_t id = __builtin_amdgcn_alignbit(p[i * step - 1], p[i * step], sh) & mask;
          bits |= ((lut[id >> 5] >> (id & 31u)) & 1u) << i;
        }
      }
    }  // filter columns are always staged (pa_query_prepare), so there is no lazy filter-decode path
  } else if (L.kind == PA_LEAF_RAW_SET) {  // coalesced loads of the raw values, a set lookup each
    const int64_t d0 = doc_base + lane;
    for (int i = 0; i < STEPS; ++i) {
      bool m;
      switch (L.vtype) {
        case PA_INT: m = raw_set_has(L, (int64_t)gp((const int32_t*)L.raw)[d0 + i * kWave]); break;
        case PA_LONG: m = raw_set_has(L, gp((const int64_t*)L.raw)[d0 + i * kWave]); break;
        case PA_FLOAT: m = raw_set_has(L, (double)gp((const float*)L.raw)[d0 + i * kWave]); break;
        default: m = raw_set_has(L, gp((const double*)L.raw)[d0 + i * kWave]); break;
      }
      bits |= (uint32_t)m << i;
    }
  } else {  // PA_LEAF_RAW_RANGE: coalesced loads of the raw values
    const int64_t d0 = doc_base + lane;
    switch (L.vtype) {
      case PA_INT: {
        const AS1 int32_t* v = gp((const int32_t*)L.raw) + d0;
#pragma unroll 8
        for (int i = 0; i < STEPS; ++i) {
          const int64_t x = v[i * kWave];
          bits |= (uint32_t)(x >= L.ilo && x <= L.ihi) << i;
        }
      } break;
      case PA_LONG: {
        const AS1 int64_t* v = gp((const int64_t*)L.raw) + d0;
#pragma unroll 8
        for (int i = 0; i < STEPS; ++i) {
          const int64_t x = v[i * kWave];
          bits |= (uint32_t)(x >= L.ilo && x <= L.ihi) << i;
        }
      } break;
      case PA_FLOAT: {
        const AS1 float* v = gp((const float*)L.raw) + d0;
#pragma unroll 8
        for (int i = 0; i < STEPS; ++i) {
          const double x = v[i * kWave];
          bits |= (uint32_t)(x >= L.dlo && x <= L.dhi) << i;
        }
      } break;
      default: {
        const AS1 double* v = gp((const double*)L.raw) + d0;
#pragma unroll 8
        for (int i = 0; i < STEPS; ++i) {
          const double x = v[i * kWave];
          bits |= (uint32_t)(x >= L.dlo && x <= L.dhi) << i;
        }
      } break;
    }
  }
  return L.negate ? ~bits : bits;
}

// A wave-uniform pointer the compiler may hold in VGPRs: readfirstlane puts it in SGPRs, so the descriptor fields
// behind it are scalar loads (vector loads of descriptors need vmcnt waits, which also wait for the in-flight DMA ring).
template <class T>
__device__ __forceinline__ T* uniform_ptr(T* p) {
  const uint64_t v = (uint64_t)p;
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return (T*)(((uint64_t)hi << 32) | lo);
}

// One literal on one doc, read straight from HBM: the lazy clauses, evaluated only on docs every eager clause
// matched (the leap-frog evaluation of the reference's AndDocIdIterator: later iterators only advance to candidate
// docs). DICT_RANGE bounds are stored MSB-aligned for leaf_bits; lo = lo' >> (32-nb), span = (hi' + 1) >> (32-nb).
__device__ __forceinline__ bool leaf_match_doc(const DevLeaf& L, int64_t doc) {
  bool m;
  if (L.kind == PA_LEAF_MV_DICT_RANGE || L.kind == PA_LEAF_MV_DICT_SET) {
    // MVScanDocIdIterator + applyMV: ANY value in the leaf's set (exclusive predicates arrive negated, so that is
    // NOT ANY == ALL values outside the set). Plain (not MSB-aligned) bounds for MV ranges.
    const int32_t v0 = gp(L.mv_off)[doc], v1 = gp(L.mv_off)[doc + 1];
    m = false;
    for (int32_t v = v0; v < v1 && !m; ++v) {
      const uint32_t id = decode_global(L.words, v, L.nbits);
      m = L.kind == PA_LEAF_MV_DICT_RANGE ? (id - (uint32_t)L.lo) < (uint32_t)L.span
                                          : ((gp(L.lut)[id >> 5] >> (id & 31u)) & 1u) != 0;
    }
  } else if (L.kind == PA_LEAF_DICT_RANGE || L.kind == PA_LEAF_DICT_SET) {
    const uint32_t id = decode_global(L.words, doc, L.nbits);
    if (L.kind == PA_LEAF_DICT_RANGE) {
      const int sh = 32 - L.nbits;
      const uint32_t lo = (uint32_t)L.lo >> sh;
      const uint32_t span = (uint32_t)(((uint64_t)(uint32_t)L.span + 1u) >> sh);
      m = (id - lo) < span;
    } else {
      m = (gp(L.lut)[id >> 5] >> (id & 31u)) & 1u;
    }
  } else if (L.kind == PA_LEAF_RAW_SET) {
    switch (L.vtype) {
      case PA_INT: m = raw_set_has(L, (int64_t)gp((const int32_t*)L.raw)[doc]); break;
      case PA_LONG: m = raw_set_has(L, gp((const int64_t*)L.raw)[doc]); break;
      case PA_FLOAT: m = raw_set_has(L, (double)gp((const float*)L.raw)[doc]); break;
      default: m = raw_set_has(L, gp((const double*)L.raw)[doc]); break;
    }
  } else {
    switch (L.vtype) {
      case PA_INT: { const int64_t x = gp((const int32_t*)L.raw)[doc]; m = x >= L.ilo && x <= L.ihi; } break;
      case PA_LONG: { const int64_t x = gp((const int64_t*)L.raw)[doc]; m = x >= L.ilo && x <= L.ihi; } break;
      case PA_FLOAT: { const double x = gp((const float*)L.raw)[doc]; m = x >= L.dlo && x <= L.dhi; } break;
      default: { const double x = gp((const double*)L.raw)[doc]; m = x >= L.dlo && x <= L.dhi; } break;
    }
  }
  return m != (L.negate != 0);
}

// ---------------------------------------------------------------- fused execution statistics (DevQuery::leap_mode)
// The filter is an AND of two single-value scan leaves: literal 0 (eager, E) and literal 1 (lazy, Z). The reference's
// AndDocIdIterator leap-frogs them with A = Z and B = E (filter_stats._cost_next: numEntriesScannedInFilter = num_docs +
// |A & B| + leaps). Label every doc A-only (1), B-only (2), both (3); in doc order a leap starts at each step
// both -> A-only, start -> A-only, A-only -> B-only and B-only -> A-only between consecutive labelled docs
// (pa_kernels.hip word_leaps). Every such step but the first has an E (= B) doc at one end, so
//   leaps = [the segment's first labelled doc is A-only]
//         + sum over E docs e of ([succ(e) is A-only] + [e is B-only and pred(e) is A-only]),
// with pred / succ the nearest labelled docs before / after e. The scan knows e's label (the lazy clause runs on it) and
// appends (segment, doc, label) to a list (leap_tile); after the scan, leap_search_kernel (pa_kernels.hip) gives every
// listed doc one wave: a wave-wide search over 64 docs per step, both leaves read straight from HBM, stops at the first
// labelled doc (so never past the neighbouring E doc) — in the scan itself every search step's load would wait behind
// the tile ring's in-flight DMA. The planner enables this only for a sparse E; a search that gives up
// (kLeapSearchSteps) or a full list flags the segment(s), whose counts the host then takes from leaf bitmaps.
// leap_out: [3 s]: segment s's matched docs, leaps, gave-up flag; [3 nseg]: list overflow flag; [3 nseg + 1 + w]: the
// docs wave w of the scan listed; then the list: wave w's slice of leap_cap entries at [3 nseg + 1 + slices + w cap],
// one (segment << 40 | doc << 1 | both) per E doc (a wave appends to its own slice: no atomic, no wait).
constexpr int kLeapSearchSteps = 64;  // 4096 docs

// Label of the nearest labelled doc at or beyond `from` in direction dir (+1 / -1) inside the segment: 1, 2, 3; 0 if
// the segment ends first; 4 if the search gave up. (Four rows of 64 docs per step measured slower: 51 vs 34 us for
// configs[1]'s list, r04_d1.)
__device__ __noinline__ uint32_t leap_search(const DevSeg* seg_in, int64_t from, int dir, int lane) {
  const DevSeg* __restrict__ seg = uniform_ptr(seg_in);
  const int64_t n = seg->num_docs;
  for (int k = 0; k < kLeapSearchSteps; ++k) {
    const int64_t d = from + (int64_t)dir * (int64_t)(kWave * k + lane);
    const bool in = d >= 0 && d < n;
    uint32_t lbl = 0u;
    if (in) lbl = (leaf_match_doc(seg->leaves[1], d) ? 1u : 0u) | (leaf_match_doc(seg->leaves[0], d) ? 2u : 0u);
    const uint64_t hit = __ballot(lbl != 0u);
    if (hit) return (uint32_t)__builtin_amdgcn_readlane((int)lbl, __builtin_ctzll(hit));  // lane order = distance
    if (__ballot(in) != ~0ull) return 0u;
  }
  return 4u;
}

// One segment's counters (lane 0 adds them; nothing when all are zero).
__device__ __forceinline__ void leap_add(const DevQuery* __restrict__ q, int seg_index, uint32_t matched, uint32_t leaps,
                                         uint32_t gave_up, int lane) {
  if (lane == 0 && (matched | leaps | gave_up)) {
    unsigned long long* o = q->leap_out + 3 * (int64_t)seg_index;
    if (matched) atomicAdd(o, (unsigned long long)matched);
    if (leaps) atomicAdd(o + 1, (unsigned long long)leaps);
    if (gave_up) atomicOr(o + 2, 1ull);
  }
}

// The E docs of one tile (e: eager clause bits, f: those that also matched the lazy clause) into the list, and the
// tile's matched docs into the segment's counter. LM: doc of bit i of lane l = 32 l + i, else 64 i + l.
template <int LM>
__device__ __forceinline__ void leap_tile(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg, int64_t doc_base,
                                       uint32_t e, uint32_t f, int lane, uint32_t slice, uint32_t& listed,
                                       uint32_t lds_base) {
  const uint32_t mine = (uint32_t)__builtin_popcount(e);
  uint32_t incl = mine;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)incl, o, kWave);
    if (lane >= o) incl += t;
  }
  const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);
  uint32_t matched = (uint32_t)__builtin_popcount(f);
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) matched += (uint32_t)__shfl_xor((int)matched, o, kWave);
  const int si = seg->index;
  const int64_t nseg = q->num_segments;
  const uint64_t cap = (uint64_t)q->leap_cap;
  if ((uint64_t)listed + total > cap) {
    if (lane == 0) atomicOr(q->leap_out + 3 * nseg, 1ull);  // (the host then takes every segment's counts from bitmaps)
  } else {
    AS1 unsigned long long* list =
        gp(q->leap_out) + 3 * nseg + 1 + (int64_t)q->leap_slices + (int64_t)slice * (int64_t)cap;
    const uint32_t lcap = (uint32_t)q->leap_lds_cap;
    lds_u64_t* lds_list = (lds_u64_t*)(uintptr_t)lds_base;
    uint32_t pos = listed + (incl - mine);
    while (e) {
      const int i = __builtin_ctz(e);
      e &= e - 1u;
      const int64_t doc = doc_base + (LM ? 32 * lane + i : kWave * i + lane);
      const uint64_t ent = ((uint64_t)si << 40) | ((uint64_t)doc << 1) | ((f >> i) & 1u);
      if (pos < lcap) lds_list[pos] = ent;
      else list[pos] = ent;
      ++pos;
    }
  }
  listed += total;
  leap_add(q, si, matched, 0u, 0u, lane);
}

// Batched decodes (part_tile in pa_strat_part.h, the lane strategy): every load of a batch is issued before any of their results is used. (A load whose
// result is consumed inside a per-lane branch gets its wait inside that branch: the batch's round trips serialise.)
// Packed values idx[i] of the stream `words` (nb bits each) for the lanes with on[i]; 0 elsewhere.
template <int N>
__device__ __forceinline__ void decode_global_batch(const uint32_t* words, const int64_t (&idx)[N], const bool (&on)[N],
                                                    int nb, uint32_t (&out)[N]) {
  uint32_t lo[N], hi[N], sh[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const uint64_t e1 = (uint64_t)idx[i] * (uint64_t)nb + (uint64_t)(nb - 1);
    const int64_t we = (int64_t)(e1 >> 5);
    sh[i] = (~(uint32_t)e1) & 31u;
    lo[i] = hi[i] = 0u;
    if (on[i]) {
      lo[i] = gp(words)[we];
      hi[i] = gp(words)[we - 1];
    }
  }
  const uint32_t mask = nbits_mask(nb);
#pragma unroll
  for (int i = 0; i < N; ++i) out[i] = on[i] ? (__builtin_amdgcn_alignbit(hi[i], lo[i], sh[i]) & mask) : 0u;
}

// dictIds of the docs of steps h .. h+N-1 (match bits m) of a column: from the staged tile image (region `loff`; every
// doc of the batch lies in the image, so all are read and the matching ones kept) or, lazily, from HBM.
template <int N, int LM>
__device__ __forceinline__ void decode_batch(int loff, int nb, const uint32_t* words, const uint32_t* img,
                                             int64_t doc_base, int h, uint32_t m, int lane, uint32_t (&id)[N]) {
  auto local = [&](int i) { return LM ? 32 * lane + i : i * kWave + lane; };
  if (loff >= 0) {
    const uint32_t* region = img + loff;
    const uint32_t mask = nbits_mask(nb);
    uint32_t lo[N], hi[N], sh[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const uint32_t e1 = (uint32_t)local(h + i) * (uint32_t)nb + (uint32_t)(nb - 1);
      const int we = (int)(e1 >> 5);
      lo[i] = region[we];
      hi[i] = region[we - 1];
      sh[i] = (~e1) & 31u;
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
      id[i] = ((m >> (h + i)) & 1u) ? (__builtin_amdgcn_alignbit(hi[i], lo[i], sh[i]) & mask) : 0u;
  } else {
    int64_t idx[N];
    bool on[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      idx[i] = doc_base + local(h + i);
      on[i] = (m >> (h + i)) & 1u;
    }
    decode_global_batch<N>(words, idx, on, nb, id);
  }
}

// Element i (wave-uniform) of a register array without dynamic register indexing.
template <int N, class T>
__device__ __forceinline__ T pick(const T (&a)[N], int i) {
  T r = a[0];
#pragma unroll
  for (int k = 1; k < N; ++k) r = i == k ? a[k] : r;
  return r;
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, kWave));
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// numGroupsLimit (walk form): the docs of match words m whose table-wide group key is admitted in this segment
// (seg->admit, written by limit_walk_kernel). Eight steps per batch: every dictId decode, then every remap gather, then
// every bitmap gather (their latencies overlap).
template <int LM, int STEPS>
__device__ __forceinline__ uint32_t admitted_docs(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                                  const uint32_t* img, int64_t doc_base, uint32_t m, int lane) {
  auto local = [&](int i) { return LM ? 32 * lane + i : i * kWave + lane; };
  const uint32_t* adm = seg->admit;
  const int ngb = q->num_gb;
  constexpr int kB = 8;
#pragma unroll 1
  for (int h = 0; h < STEPS; h += kB) {
    if (__ballot(((m >> h) & 0xffu) != 0) == 0) continue;
    uint32_t key[kB];
#pragma unroll
    for (int i = 0; i < kB; ++i) key[i] = 0u;
    for (int j = 0; j < ngb; ++j) {
      const DevCol& c = seg->cols[q->gb_slot[j]];
      const int32_t* rm = seg->remap[j];
      const uint32_t st = (uint32_t)q->gb_stride[j];
      uint32_t id[kB];
#pragma unroll
      for (int i = 0; i < kB; ++i) {
        id[i] = 0u;
        if ((m >> (h + i)) & 1u) id[i] = decode_dict_id<false>(c, img, local(h + i), doc_base + local(h + i));
      }
      if (rm != nullptr) {
#pragma unroll
        for (int i = 0; i < kB; ++i)
          if ((m >> (h + i)) & 1u) id[i] = (uint32_t)gp(rm)[id[i]];
      }
#pragma unroll
      for (int i = 0; i < kB; ++i) key[i] += id[i] * st;  // direct key space of at most kWalkMaxKeys keys
    }
    uint32_t w[kB];
#pragma unroll
    for (int i = 0; i < kB; ++i) w[i] = ((m >> (h + i)) & 1u) ? gp(adm)[key[i] >> 5] : 0u;
#pragma unroll
    for (int i = 0; i < kB; ++i)
      if (!((w[i] >> (key[i] & 31u)) & 1u)) m &= ~(1u << (h + i));
  }
  return m;
}

// ---------------------------------------------------------------- strategies in headers of their own
// The lane, selection, distinct, filtered-aggregation, expression and partitioned strategies live in pa_strat_*.h,
// which this header does not include: their entry points are declared here, each call below sits in an `if constexpr`,
// and a unit includes the pa_strat_*.h of the strategies it instantiates (each includes this header). An edit to one of
// them so rebuilds that strategy's units only.
// pa_strat_lane.h
__device__ __forceinline__ void lane_acc_init(const DevQuery* __restrict__ q, WaveState& la, const void* lds_area,
                                              int wgs);
__device__ __forceinline__ void lane_acc_segment_end(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                                     WaveState& la, bool any);
template <int LM, int STEPS, int STRAT>
__device__ __forceinline__ void lane_acc_tile(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                              const uint32_t* img, int64_t doc_base, uint32_t m, int lane,
                                              WaveState& la, unsigned char* lds);
__device__ __forceinline__ void lane_acc_flush(const DevQuery* __restrict__ q, const WaveState& la, int lane);
template <int WGS>
__device__ __forceinline__ void lane_hist_zero(const DevQuery* q, unsigned char* lds_acc);
template <int WGS>
__device__ __forceinline__ void lane_hist_fold(const DevQuery* q, const DevSeg* segs, unsigned char* lds_acc,
                                               const WaveState& la);
// pa_strat_select.h
template <int STEPS, int LM>
__device__ __forceinline__ void select_tile(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                            const uint32_t* img, int64_t doc_base, uint32_t m, int lane, WaveState& la);
__device__ __forceinline__ void sel_state_init(WaveState& la, const uint32_t* smem, int wave);
__device__ __forceinline__ void sel_segment_docs(const DevQuery* q, const DevSeg* seg, uint32_t matched,
                                                 uint32_t matched_seg0, int lane);
__device__ __forceinline__ void sel_counters_flush(const DevQuery* q, const WaveState& la, int lane);
// pa_strat_distinct.h
template <int STRAT, int STEPS, int LM>
__device__ __forceinline__ void distinct_tile(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                              const uint32_t* img, int64_t doc_base, uint32_t m, int lane,
                                              unsigned char* lds);
template <int WGS>
__device__ __forceinline__ void distinct_lds_zero(const DevQuery* q, unsigned char* lds);
template <int WGS>
__device__ __forceinline__ void distinct_lds_flush(const DevQuery* q, unsigned char* lds);
// pa_strat_filtered.h
template <int STRAT, int STEPS>
__device__ __forceinline__ void filtered_tile(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                              const uint32_t* img, int64_t doc_base, uint32_t m, int lane,
                                              const Acc<STRAT>& acc);
template <int WGS>
__device__ __forceinline__ void filtered_lds_zero(const DevQuery* q, unsigned char* lds_acc);
template <int WGS>
__device__ __forceinline__ void filtered_lds_flush(const DevQuery* q, unsigned char* lds_acc);
// pa_strat_expr.h
template <int STRAT>
__device__ __forceinline__ void expr_step(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                          const uint32_t* img, int doc_local, int64_t doc, uint64_t matched, int lane,
                                          const Acc<STRAT>& acc);
// pa_strat_trow.h
template <int STRAT>
__device__ __forceinline__ void trow_step(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                          const uint32_t* img, int doc_local, int64_t doc, uint64_t matched, int lane,
                                          const Acc<STRAT>& acc);
template <int WGS>
__device__ __forceinline__ void trow_lds_zero(const DevQuery* q, unsigned char* lds_acc);
template <int WGS>
__device__ __forceinline__ void trow_lds_flush(const DevQuery* q, unsigned char* lds_acc);
// pa_strat_moments.h
template <int STRAT>
__device__ __forceinline__ void mom_step(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                         const uint32_t* img, int doc_local, int64_t doc, uint64_t matched, int lane,
                                         const Acc<STRAT>& acc);
template <int WGS>
__device__ __forceinline__ void mom_lds_zero(const DevQuery* q, unsigned char* lds_acc);
template <int WGS>
__device__ __forceinline__ void mom_lds_flush(const DevQuery* q, unsigned char* lds_acc);
// pa_strat_part.h
template <int STRAT, int STEPS, int LM>
__device__ __forceinline__ void part_tile(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                          const uint32_t* img, int64_t doc_base, uint32_t m, int lane,
                                          unsigned char* lds, const PartScratch& ps);
template <int WGS>
__device__ __forceinline__ void pcount_zero(const DevQuery* q, unsigned char* lds_acc);
template <int WGS>
__device__ __forceinline__ void pcount_store(const DevQuery* q, unsigned char* lds_acc, const PartScratch& ps,
                                             int64_t lb);
template <int WGS>
__device__ __forceinline__ void pemit_begin(const DevQuery* q, unsigned char* lds_acc, const PartScratch& ps);
template <int WGS>
__device__ __forceinline__ void pemit_finish(const DevQuery* q, unsigned char* lds_acc, const PartScratch& ps,
                                             int64_t lb);

// The rare part of a tile (some doc survived the eager clauses): lazy clauses per surviving doc, then aggregation.
// Returns the docs that matched.
// LM: doc of bit i of lane l = 32l + i (lane-major tile), else 64i + l.
template <int STRAT, int STEPS, int LM>
__device__ __forceinline__ uint32_t tile_survivors(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg_in,
                                                const uint32_t* img, int64_t doc_base, uint32_t m, int lane,
                                                unsigned char* lds, const PartScratch& ps, WaveState& la) {
  const DevSeg* __restrict__ seg = uniform_ptr(seg_in);
  doc_base = ((int64_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)doc_base >> 32)) << 32) |
             (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)doc_base);
  const Acc<STRAT> acc{q, lds, &ps};
  auto local = [&](int i) { return LM ? 32 * lane + i : i * kWave + lane; };
  const int nleaves = q->num_leaves;
  const int neager = q->num_eager;
  if (neager < nleaves) {
    const uint32_t eager = m;
    // lazy clauses: only the docs the eager clauses kept, one step at a time, straight from HBM
    for (int i = 0; i < STEPS; ++i) {
      const uint32_t bit = 1u << i;
      if (__ballot((m & bit) != 0) == 0) continue;
      const int64_t doc = doc_base + local(i);
      bool ok = (m & bit) != 0;
      bool any = false;
      for (int li = neager; li < nleaves; ++li) {
        const DevLeaf& L = seg->leaves[li];
        if (ok && !any) any = leaf_match_doc(L, doc);
        if (L.clause_end) {
          ok = ok && any;
          any = false;
        }
      }
      if (!ok) m &= ~bit;
    }
    if constexpr (!is_pcount(STRAT) && !is_pemit(STRAT))
      if (q->leap_mode) leap_tile<LM>(q, seg, doc_base, eager, m, lane, la.leap_slice, la.leap_n, la.leap_lds);
    if (__ballot(m != 0) == 0) return 0;
  }
  const uint32_t scanned = m;  // numDocsScanned counts every doc the filter kept, admitted or not
  // (an MV group-by admits (doc, value) keys one by one: accumulate_doc_mv, mv_key_records)
  if (seg->admit != nullptr && q->gb_mv < 0) {
    m = admitted_docs<LM, STEPS>(q, seg, img, doc_base, m, lane);
    if (__ballot(m != 0) == 0) return (uint32_t)__builtin_popcount(scanned);
  }
  if constexpr (STRAT == STRAT_SELECT) {
    select_tile<STEPS, LM>(q, seg, img, doc_base, m, lane, la);
  } else if constexpr (is_distinct(STRAT)) {
    distinct_tile<STRAT, STEPS, LM>(q, seg, img, doc_base, m, lane, lds);
  } else if constexpr (is_filtered(STRAT)) {
    static_assert(!LM, "filtered aggregations run step-major tiles");
    filtered_tile<STRAT, STEPS>(q, seg, img, doc_base, m, lane, acc);
  } else if constexpr (is_expr(STRAT)) {
    static_assert(!LM, "expression queries run step-major tiles");
    for (int i = 0; i < STEPS; ++i) {
      const uint64_t sm = __ballot((m >> i) & 1u);
      if (sm == 0) continue;
      expr_step<STRAT>(q, seg, img, i * kWave + lane, doc_base + i * kWave + lane, sm, lane, acc);
    }
  } else if constexpr (is_trow(STRAT)) {
    static_assert(!LM, "row-by-time queries run step-major tiles");
    for (int i = 0; i < STEPS; ++i) {
      const uint64_t sm = __ballot((m >> i) & 1u);
      if (sm == 0) continue;
      trow_step<STRAT>(q, seg, img, i * kWave + lane, doc_base + i * kWave + lane, sm, lane, acc);
    }
  } else if constexpr (is_mom(STRAT)) {
    static_assert(!LM, "moment queries run step-major tiles");
    for (int i = 0; i < STEPS; ++i) {
      const uint64_t sm = __ballot((m >> i) & 1u);
      if (sm == 0) continue;
      mom_step<STRAT>(q, seg, img, i * kWave + lane, doc_base + i * kWave + lane, sm, lane, acc);
    }
  } else if constexpr (is_lane(STRAT)) {
    if constexpr (STRAT != STRAT_LANE_CNT) lane_acc_tile<LM, STEPS, STRAT>(q, seg, img, doc_base, m, lane, la, lds);
  } else if constexpr (is_pcount(STRAT) || is_pemit(STRAT)) {
    part_tile<STRAT, STEPS, LM>(q, seg, img, doc_base, m, lane, lds, ps);
  } else if (q->has_mv) {
    for (int i = 0; i < STEPS; ++i)
      if ((m >> i) & 1u) accumulate_doc_mv<STRAT>(q, seg, img, local(i), doc_base + local(i), acc);
  } else if constexpr (STRAT == STRAT_LDS && LM) {
    // matches of the wave's tile: a dense tile whose aggregations all read one raw column takes that column's tile as
    // coalesced loads; else per-lane batches, 8 docs deep when most lanes have that many (more gathers in flight)
    uint32_t tot = (uint32_t)__builtin_popcount(m);
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) tot += (uint32_t)__shfl_xor((int)tot, o, kWave);
    const int rs = q->hashed ? -1 : q->lds_raw_slot;
    if (tot > 256u && rs >= 0 && seg->cols[rs].kind == COL_SV_RAW) {
      const int vt = seg->cols[rs].vtype;
      if (vt == PA_INT || vt == PA_FLOAT) accumulate_lds_raw_dense<4>(q, seg, img, doc_base, m, lane, lds);
      else accumulate_lds_raw_dense<8>(q, seg, img, doc_base, m, lane, lds);
    } else if (tot > 512u) {
      accumulate_lds_lm<8>(q, seg, img, doc_base, m, lane, lds);
    } else {
      accumulate_lds_lm<4>(q, seg, img, doc_base, m, lane, lds);
    }
  } else {
    for (int i = 0; i < STEPS; ++i) {
      const uint64_t sm = __ballot((m >> i) & 1u);
      if (sm == 0) continue;
      accumulate_step<STRAT>(q, seg, img, local(i), doc_base + local(i), sm, lane, acc);
    }
  }
  __builtin_amdgcn_s_waitcnt((7 << 4) | (15 << 8));  // vmcnt(0): no compiler-visible load left pending
  return (uint32_t)__builtin_popcount(scanned);
}

template <int STRAT, int STEPS>
__device__ __forceinline__ void process_tile(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                             int64_t wt, const uint32_t* img, int lane, const Acc<STRAT>& acc,
                                             uint32_t& matched, WaveState& la) {
  const int64_t doc_base = wt * (STEPS * kWave);
  // docs of this tile owned by the lane: 64*i + lane < rem
  const int64_t rem = (int64_t)seg->num_docs - doc_base;
  // bit i <=> step i holds a doc of this segment (only the low STEPS bits: a negated leaf sets the others, and the
  // matched-doc count must not see them)
  constexpr uint32_t kFull = STEPS == 32 ? 0xffffffffu : ((1u << STEPS) - 1u);
  uint32_t valid;
  if (rem >= (STEPS * kWave)) {
    valid = kFull;
  } else {
    const int64_t n = rem > lane ? (rem - lane + kWave - 1) / kWave : 0;  // steps with a valid doc for this lane
    valid = n >= 32 ? 0xffffffffu : ((1u << n) - 1u);
  }
  uint32_t m = valid;
  uint32_t clause = 0;
  const int neager = q->num_eager;
  for (int li = 0; li < neager; ++li) {
    const DevLeaf& L = seg->leaves[li];
    clause |= leaf_bits<STEPS>(L, img, doc_base, lane);
    if (L.clause_end) {
      m &= clause;
      clause = 0;
      if (__ballot(m != 0) == 0) return;  // no doc of the tile can match any more
    }
  }
  if (__ballot(m != 0) == 0) return;
  matched += tile_survivors<STRAT, STEPS, 0>(q, seg, img, doc_base, m, lane, acc.lds, *acc.ps, la);
}


// ---------------------------------------------------------------- lane-major tile evaluation (scan_kernel<.., LM=1>)
//
// Lane l owns docs [32l, 32l+32) of the wave tile, i.e. the nb consecutive stream words [l*nb, (l+1)*nb) of every
// staged column: an eager leaf is nb ds_reads at immediate offsets (1x the staged bytes, against 2 dwords per doc in
// the step-major layout) plus a static unpack (nb is a template parameter: every shift is a constant).

__device__ __forceinline__ uint32_t rl(uint32_t v, int k) { return (uint32_t)__builtin_amdgcn_readlane((int)v, k); }

// Match word of one DICT_RANGE / DICT_SET leaf: bit i <=> doc 32*lane + i of the tile matches (before negation).
template <int NB>
__device__ __forceinline__ uint32_t leaf_lm(int kind, uint32_t region_lds, int lane, uint32_t lo_t, uint32_t hi_t,
                                            const uint32_t* lut) {
  const lds_u32_t* p = (const lds_u32_t*)(uintptr_t)(region_lds + (uint32_t)lane * (uint32_t)(NB * 4));
  // Wide columns are unpacked in two halves of 16 docs, so at most ~NB/2 + 1 stream words are live at once (keeps
  // the kernel within 128 VGPRs: 4 waves per SIMD).
  constexpr int H = NB > 16 ? 2 : 1;
  constexpr int DPH = 32 / H;  // docs per half
  uint32_t nm = 0, bits = 0;
#pragma unroll
  for (int h = H - 1; h >= 0; --h) {
    constexpr int WMAX = (DPH * NB + 31) / 32 + 1;
    const int wlo = (h * DPH * NB) >> 5;  // first stream word of this half (compile-time after unrolling)
    uint32_t w[WMAX];
#pragma unroll
    for (int j = 0; j < WMAX; ++j) w[j] = (wlo + j < NB) ? p[wlo + j] : 0u;
    // MSB-aligned value of doc i: the NB bits starting at stream bit i*NB, in the top bits of t
    auto top = [&](int i) -> uint32_t {
      const int s = i * NB, j = (s >> 5) - wlo, o = s & 31;
      if (o + NB <= 32) return w[j] << o;
      return __builtin_amdgcn_alignbit(w[j], w[(j + 1 < WMAX) ? j + 1 : j], 32 - o);
    };
    if (kind == PA_LEAF_DICT_RANGE) {
      // lo <= v < lo + span  <=>  (t - lo') <= hi' (unsigned), lo' / hi' MSB-aligned by the host (see leaf_bits);
      // non-matches accumulate as nm = 2*nm + borrow: bit i of nm = doc i does not match
#pragma unroll
      for (int i = (h + 1) * DPH - 1; i >= h * DPH; --i) {
        const uint32_t t = top(i);
        uint32_t u;
        asm("v_sub_u32_e64 %[u], %[t], %[lo]\n\t"
            "v_sub_co_u32_e32 %[u], vcc, %[hi], %[u]\n\t"
            "v_addc_co_u32_e32 %[nm], vcc, %[nm], %[nm], vcc"
            : [nm] "+v"(nm), [u] "=&v"(u)
            : [t] "v"(t), [lo] "s"(lo_t), [hi] "s"(hi_t)
            : "vcc");
      }
    } else {
      const AS1 uint32_t* lt = gp(lut);
#pragma unroll
      for (int i = h * DPH; i < (h + 1) * DPH; ++i) {
        const uint32_t id = top(i) >> (32 - NB);
        bits |= ((lt[id >> 5] >> (id & 31u)) & 1u) << i;
      }
    }
  }
  return kind == PA_LEAF_DICT_RANGE ? ~nm : bits;
}

__device__ __forceinline__ uint32_t leaf_lm_any(int nb, int kind, uint32_t region_lds, int lane, uint32_t lo_t,
                                                uint32_t hi_t, const uint32_t* lut) {
  switch (nb) {
#define PA_LM_CASE(N) \
  case N: return leaf_lm<N>(kind, region_lds, lane, lo_t, hi_t, lut);
    PA_LM_CASE(1) PA_LM_CASE(2) PA_LM_CASE(3) PA_LM_CASE(4) PA_LM_CASE(5) PA_LM_CASE(6) PA_LM_CASE(7) PA_LM_CASE(8)
    PA_LM_CASE(9) PA_LM_CASE(10) PA_LM_CASE(11) PA_LM_CASE(12) PA_LM_CASE(13) PA_LM_CASE(14) PA_LM_CASE(15)
    PA_LM_CASE(16) PA_LM_CASE(17) PA_LM_CASE(18) PA_LM_CASE(19) PA_LM_CASE(20) PA_LM_CASE(21) PA_LM_CASE(22)
    PA_LM_CASE(23) PA_LM_CASE(24) PA_LM_CASE(25) PA_LM_CASE(26) PA_LM_CASE(27) PA_LM_CASE(28) PA_LM_CASE(29)
    PA_LM_CASE(30) PA_LM_CASE(31) PA_LM_CASE(32)
#undef PA_LM_CASE
    default: return 0;
  }
}

// Equality prefilter of a full lane-major tile (pa_eq_any.h): non-zero iff one of the lane's 32 docs has the dictId of
// the pattern `window`. Never a match word: a tile where no lane answers non-zero is done, any other goes through
// leaf_lm_any as before. Widths above kEqPrefilterMaxNb (pa_device.h) are not compiled: the planner never asks.
__device__ __forceinline__ uint32_t eq_any_lm(int nb, uint32_t region_lds, int lane, uint64_t window) {
  // The pattern words are shifts of the window, one scalar instruction each. Opaque here, so that they are taken per
  // tile: hoisted out of the tile loop they are nb more live scalar registers, which the kernel does not have (they
  // came back per tile as v_readlane pairs from a spill register, vector instructions the prefilter is there to save).
  asm volatile("" : "+s"(window));
  switch (nb) {
#define PA_EQ_CASE(N)                                                                                        \
  case N: {                                                                                                  \
    const lds_u32_t* p = (const lds_u32_t*)(uintptr_t)(region_lds + (uint32_t)lane * (uint32_t)(N * 4));     \
    return eq_any<N>([p](int j) -> uint32_t { return p[j]; }, window);                                       \
  }
    PA_EQ_CASE(1) PA_EQ_CASE(2) PA_EQ_CASE(3) PA_EQ_CASE(4) PA_EQ_CASE(5) PA_EQ_CASE(6) PA_EQ_CASE(7) PA_EQ_CASE(8)
    PA_EQ_CASE(9) PA_EQ_CASE(10) PA_EQ_CASE(11) PA_EQ_CASE(12) PA_EQ_CASE(13) PA_EQ_CASE(14) PA_EQ_CASE(15)
    PA_EQ_CASE(16) PA_EQ_CASE(17) PA_EQ_CASE(18) PA_EQ_CASE(19) PA_EQ_CASE(20) PA_EQ_CASE(21) PA_EQ_CASE(22)
    PA_EQ_CASE(23) PA_EQ_CASE(24)
#undef PA_EQ_CASE
    default: return 1u;  // (not compiled: every tile takes the leaf)
  }
}
static_assert(kEqPrefilterMaxNb == 24, "eq_any_lm compiles the widths 1..kEqPrefilterMaxNb");

// LDS-DMA of one wave tile of every staged column (plan table `ip`), padded to exactly D instructions.
__device__ __forceinline__ void stage_tile_lm(uint32_t ip, int64_t wt, uint32_t img_lds, int lane, const int D) {
  const int ns = (int)rl(ip, 0);
  int issued = 0;
  for (int c = 0; c < ns; ++c) {
    const uint64_t words = ((uint64_t)rl(ip, 9 + 4 * c) << 32) | rl(ip, 8 + 4 * c);
    const int nb = (int)rl(ip, 10 + 4 * c);
    const uint32_t dst = img_lds + 4u * rl(ip, 11 + 4 * c);
    const char* src = (const char*)words + wt * (int64_t)(256 * nb) + 16 * lane;  // 256*nb bytes per wave tile
    const int chunks = 16 * nb;                                                      // 16-byte chunks per wave tile
    for (int c0 = 0; c0 < chunks; c0 += 64) {
      if (c0 + lane < chunks) dma16(src + 16 * c0, dst + 16 * c0);
      ++issued;
    }
  }
  const void* dummy = (const void*)(((uint64_t)rl(ip, 5) << 32) | rl(ip, 4));
  for (; issued < D; ++issued) {
    if (lane == 0) dma16(dummy, img_lds);
  }
}

template <int STRAT>
__device__ __forceinline__ void process_tile_lm(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                                uint32_t pp, int64_t wt, const uint32_t* img, uint32_t img_lds,
                                                int lane, const Acc<STRAT>& acc, uint32_t& matched, WaveState& la) {
  const int64_t doc_base = wt * kWTileDocs;
  const int64_t rem = (int64_t)(int32_t)rl(pp, 2) - doc_base;
  uint32_t valid = 0xffffffffu;
  if (rem < kWTileDocs) {
    const int64_t n = rem - 32 * lane;  // docs of this lane's 32 that exist
    valid = n >= 32 ? 0xffffffffu : (n <= 0 ? 0u : ((1u << n) - 1u));
  }
  uint32_t m = valid;
  uint32_t clause = 0;
  const int neager = (int)rl(pp, 1);
  for (int l = 0; l < neager; ++l) {
    const int b = 24 + 8 * l;
    const int flags = (int)rl(pp, b + 5);
    const uint32_t* lut = (const uint32_t*)(((uint64_t)rl(pp, b + 7) << 32) | rl(pp, b + 6));
    uint32_t bits = leaf_lm_any((int)rl(pp, b + 1), (int)rl(pp, b), img_lds + 4u * rl(pp, b + 2), lane,
                                rl(pp, b + 3), rl(pp, b + 4), lut);
    if (flags & 1) bits = ~bits;
    clause |= bits;
    if (flags & 2) {
      m &= clause;
      clause = 0;
      if (__ballot(m != 0) == 0) return;
    }
  }
  if (__ballot(m != 0) == 0) return;
  matched += tile_survivors<STRAT, 32, 1>(q, seg, img, doc_base, m, lane, acc.lds, *acc.ps, la);
}

__device__ __forceinline__ int find_segment(const DevSeg* __restrict__ segs, int nseg, int64_t t) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].first_wtile <= t) lo = mid;
    else hi = mid - 1;
  }
  while (t >= segs[lo].first_wtile + segs[lo].num_wtiles) ++lo;
  return lo;
}

// s_waitcnt vmcnt(N) that also "produces" `token` (the ring slot's LDS offset): every LDS read of the slot is
// addressed through the token, so it cannot be scheduled above the wait. No "memory" clobber: a clobber would
// make the compiler re-load every query/segment descriptor field after each wait (dependent SMEM round trips per
// tile).
template <int N>
__device__ __forceinline__ void vm_wait_token(uint32_t& token) {
  static_assert(N >= 0 && N < 64, "vmcnt is 6 bits");
  token = (uint32_t)__builtin_amdgcn_readfirstlane((int)token);  // wave-uniform (see dma16)
  asm volatile("s_waitcnt vmcnt(%1)" : "+s"(token) : "n"(N));
}

// vmcnt(n) for a wave-uniform runtime n in [LO, HI]: a 6-deep binary tree of scalar branches down to the immediate.
template <int LO, int HI>
__device__ __forceinline__ void vm_wait_n(uint32_t& token, int n) {
  if constexpr (LO == HI) {
    vm_wait_token<LO>(token);
  } else {
    constexpr int MID = (LO + HI) / 2;
    if (n <= MID) vm_wait_n<LO, MID>(token, n);
    else vm_wait_n<MID + 1, HI>(token, n);
  }
}

// Wait until the tile with `younger` tiles issued after it has landed (every tile is exactly D DMA instructions,
// so that is vmcnt(younger * D); above 63 — the counter's width — vmcnt(63) waits for more, never less); `token` =
// the tile's slot offset.
__device__ __forceinline__ void wait_tile(int younger, int D, uint32_t& token) {
  const int n = younger * D;
  vm_wait_n<0, 63>(token, n < 63 ? n : 63);
}

// Issue side of the lane-major steady state, hoisted per segment (see scan_kernel).
struct LmIssue {
  const char* base[kLmStaged];  // column stream (wave-uniform: the lane's 16-byte offset is added per DMA)
  int64_t stride[kLmStaged];    // bytes per wave tile
  uint32_t off[kLmStaged];      // LDS byte offset of the column region in a tile image
  int nfull[kLmStaged];         // full 64-lane DMA instructions per tile
  uint64_t tail[kLmStaged];     // lanes of the last, partial instruction (0 = none)
  int nst;
  const void* dummy;
};

// Wait for the tile in slot `slot_off`, then issue the next tile `ti` (ring slot `islot`): every instruction a full
// 64-lane DMA except a column's lane-masked tail, padded to exactly D instructions.
template <bool NT = false>
__device__ __forceinline__ void lm_wait_issue(const LmIssue& I, uint32_t& slot_off, int R, int D, int64_t younger,
                                              uint32_t dst0, int64_t it, uint32_t lane_off) {
  if (R == 2) vm_wait_token<0>(slot_off);  // the one tile in flight has landed
  else wait_tile((int)younger, D, slot_off);
  int issued = 0;
#pragma unroll
  for (int c = 0; c < kLmStaged; ++c) {
    if (c < I.nst) {
      const char* src = I.base[c] + it * I.stride[c] + lane_off;
      const uint32_t dst = dst0 + I.off[c];
      for (int k = 0; k < I.nfull[c]; ++k) dma16<NT>(src + 1024 * k, dst + 1024 * k);
      issued += I.nfull[c];
      if (I.tail[c]) {
        dma16_masked<NT>(src + 1024 * I.nfull[c], dst + 1024 * I.nfull[c], I.tail[c]);
        ++issued;
      }
    }
  }
  for (; issued < D; ++issued) dma16_masked(I.dummy, dst0, 1ull);
}

// The V-only emit of 4-wave workgroups (one whole tile per batch in part_tile): compiled for 2 workgroups per CU.
__host__ __device__ constexpr bool emit_v_wide(int s) {
  return is_pemit(s) && !pemit_hh(s) && !pemit_big(s) && pemit_vf(s) != V_FMT_GEN;
}

// LM = 1: lane-major tiles (STEPS must be 32) driven by the per-segment plan tables `plans`; LM = 0: step-major.
template <int STRAT, int STEPS, int LM>
__global__ void __launch_bounds__(scan_waves(STRAT) * kWave, emit_v_wide(STRAT) ? 2 : (scan_waves(STRAT) == kWavesPerWG ? 4 : 1)) scan_kernel(const DevQuery* __restrict__ q,
                                                       const DevSeg* __restrict__ segs,
                                                       const LmSegPlan* __restrict__ plans, PartScratch ps) {
  static_assert(!LM || STEPS == 32, "lane-major tiles are 2048 docs");
  constexpr int WPW = scan_waves(STRAT);  // waves per workgroup
  constexpr int WGS = WPW * kWave;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int lane = threadIdx.x & 63;
  // wave-uniform by construction; readfirstlane makes the compiler keep the whole tile/segment cursor in SGPRs
  // (otherwise segment descriptors are read with vector loads whose vmcnt(0) waits drain the DMA ring)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  unsigned char* lds_acc = (unsigned char*)smem;
  const uint32_t acc_dwords = STRAT != STRAT_GLOBAL ? (q->lds_acc_bytes >> 2) : 0u;
  const int img_dw = q->image_dwords_max;
  uint32_t* ring = smem + acc_dwords + wave * q->ring * img_dw;
  Acc<STRAT> acc{q, lds_acc, &ps};

  if (STRAT == STRAT_LDS) lds_acc_zero<WGS>(q, lds_acc);
  else if constexpr (is_pcount(STRAT)) pcount_zero<WGS>(q, lds_acc);
  else if constexpr (is_pemit(STRAT)) pemit_begin<WGS>(q, lds_acc, ps);

  uint32_t matched = 0;  // docs of this lane that passed the filter (numDocsScanned)
  WaveState la;
  la.leap_slice = (uint32_t)((q->xcd_major ? xcd_major_block(blockIdx.x, gridDim.x) : (int64_t)blockIdx.x) * WPW + wave);
  la.leap_n = 0u;
  la.leap_lds = lds_addr(smem + acc_dwords + (uint32_t)WPW * (uint32_t)q->ring * (uint32_t)img_dw) +
                (uint32_t)wave * (uint32_t)q->leap_lds_cap * 8u;
  if constexpr (is_lane(STRAT) && STRAT != STRAT_LANE_CNT) lane_acc_init(q, la, smem, WGS);
  if constexpr (STRAT == STRAT_SELECT) sel_state_init(la, smem, wave);
  if constexpr (STRAT == STRAT_DISTINCT_LDS) distinct_lds_zero<WGS>(q, lds_acc);
  if constexpr (STRAT == STRAT_FILTERED_LDS) filtered_lds_zero<WGS>(q, lds_acc);
  if constexpr (STRAT == STRAT_EXPR_LDS) lds_acc_zero<WGS>(q, lds_acc);
  if constexpr (STRAT == STRAT_TROW_LDS) trow_lds_zero<WGS>(q, lds_acc);
  if constexpr (STRAT == STRAT_MOM_LDS) mom_lds_zero<WGS>(q, lds_acc);
  if constexpr (STRAT == STRAT_LANE_DICT) lane_hist_zero<WGS>(q, lds_acc);
  const int64_t T = q->total_wtiles;
  const int64_t W = (int64_t)gridDim.x * WPW;
  // logical block: also derived in pemit_begin and for la.leap_slice above; deriving it once changes every scan kernel's
  // registers and code size (as does moving the leap-list write-out below into a function), so the copies stay
  const int64_t lb = q->xcd_major ? xcd_major_block(blockIdx.x, gridDim.x) : (int64_t)blockIdx.x;
  const int64_t gw = lb * WPW + wave;
  const int64_t t0 = gw * T / W;
  const int64_t t1 = (gw + 1) * T / W;
  if (t0 < t1) {
    // Ring of R wave-tile images: tiles t+1 .. t+R-1 stream in (LDS-DMA) while tile t is decoded; each tile is
    // exactly D DMA instructions, so "tile t landed" is vmcnt(<= (tiles issued after t) * D).
    const int R = q->ring;
    const int D = q->dma_per_tile;
    int isi = find_segment(segs, q->num_segments, t0);   // issue cursor: segment, its tile range, ring slot
    int64_t ifirst = segs[isi].first_wtile;
    int64_t iend = ifirst + segs[isi].num_wtiles;
    // LM: the issue segment's plan table, one dword per lane (its load drains the ring once per segment crossing)
    uint32_t ip = LM ? ((const uint32_t*)(plans + isi))[lane] : 0u;
    int64_t ti = t0;
    int islot = 0;
    const uint32_t ring_lds = lds_addr(ring);
    auto issue_next = [&]() {
      while (ti >= iend) {
        ++isi;
        ifirst = segs[isi].first_wtile;
        iend = ifirst + segs[isi].num_wtiles;
        if (LM) ip = ((const uint32_t*)(plans + isi))[lane];
      }
      if constexpr (LM) stage_tile_lm(ip, ti - ifirst, ring_lds + 4u * (uint32_t)(islot * img_dw), lane, D);
      else stage_tile<STEPS>(segs + isi, ti - ifirst, ring + islot * img_dw, lane, D);
      ++ti;
      islot = islot + 1 == R ? 0 : islot + 1;
    };
    for (int k = 0; k < R - 1 && ti < t1; ++k) issue_next();

    int si = find_segment(segs, q->num_segments, t0);
    int pslot = 0;
    int64_t t = t0;
    while (t < t1) {
      // segment-outer / tile-inner: `seg` is invariant in the inner loop, so its descriptors stay in SGPRs
      const DevSeg* seg = segs + si;
      const uint32_t matched_seg0 = matched;
      const int64_t seg_first = seg->first_wtile;
      const int64_t seg_end = min(t1, seg_first + (int64_t)seg->num_wtiles);
      const uint32_t pp = LM ? ((const uint32_t*)(plans + si))[lane] : 0u;  // process segment's plan table
      const bool stream_only = q->debug_stream_only != 0;
      if constexpr (LM) {
        if (!stream_only && isi == si) {
          // Steady state: the tile to issue lies in this segment too; every per-segment value of the issue side and of
          // the leaf is hoisted into registers (no segment-crossing checks, no plan-table reads per tile).
          LmIssue I;
          I.nst = (int)rl(pp, 0);
#pragma unroll
          for (int c = 0; c < kLmStaged; ++c) {
            const int nb = c < I.nst ? (int)rl(pp, 10 + 4 * c) : 0;
            I.base[c] = (const char*)(((uint64_t)rl(pp, 9 + 4 * c) << 32) | rl(pp, 8 + 4 * c));
            I.stride[c] = 256 * (int64_t)nb;  // bytes of one wave tile of an nb-bit column
            I.off[c] = 4u * rl(pp, 11 + 4 * c);
            I.nfull[c] = (16 * nb) / 64;
            const int tail = (16 * nb) % 64;
            I.tail[c] = tail ? ((1ull << tail) - 1ull) : 0ull;
          }
          I.dummy = (const void*)(((uint64_t)rl(pp, 5) << 32) | rl(pp, 4));
          const int64_t issue_end = min(iend, t1);
          const bool single_range = (int)rl(pp, 1) == 1 && (int)rl(pp, 24) == PA_LEAF_DICT_RANGE && (rl(pp, 29) & 2u);
          if (single_range) {
            // one eager DICT_RANGE literal closing its clause: the hoisted leaf on whole tiles (the ragged last tile of
            // a segment goes through process_tile_lm)
            const int nb0 = (int)rl(pp, 25);
            const uint32_t off0 = 4u * rl(pp, 26), lo0 = rl(pp, 27), hi0 = rl(pp, 28);
            const bool neg0 = (rl(pp, 29) & 1u) != 0;
            const int64_t full_tiles = (int64_t)(int32_t)rl(pp, 2) / kWTileDocs;
            // the planner's per-segment choices (LmSegPlan::flags): the equality prefilter with its pattern, nt DMAs
            const uint32_t lmf = rl(pp, 6);
            const bool eq0 = (lmf & kLmEqPrefilter) != 0, nt = (lmf & kLmStreamNt) != 0;
            const uint64_t eq_win = ((uint64_t)rl(pp, 57) << 32) | rl(pp, 56);
            while (t < seg_end && ti < issue_end) {
              uint32_t slot_off = (uint32_t)(pslot * img_dw);
              if (nt)
                lm_wait_issue<true>(I, slot_off, R, D, ti - (t + 1), ring_lds + 4u * (uint32_t)(islot * img_dw),
                                    ti - ifirst, 16u * (uint32_t)lane);
              else
                lm_wait_issue(I, slot_off, R, D, ti - (t + 1), ring_lds + 4u * (uint32_t)(islot * img_dw), ti - ifirst,
                              16u * (uint32_t)lane);
              ++ti;
              islot = islot + 1 == R ? 0 : islot + 1;
              if (t - seg_first < full_tiles) {
                if (!eq0 || __ballot(eq_any_lm(nb0, ring_lds + 4u * slot_off + off0, lane, eq_win) != 0) != 0) {
                  uint32_t m = leaf_lm_any(nb0, PA_LEAF_DICT_RANGE, ring_lds + 4u * slot_off + off0, lane, lo0, hi0,
                                           nullptr);
                  if (neg0) m = ~m;
                  if (__ballot(m != 0) != 0)
                    matched += tile_survivors<STRAT, 32, 1>(q, seg, ring + slot_off, (t - seg_first) * kWTileDocs, m,
                                                            lane, acc.lds, *acc.ps, la);
                }
              } else {
                process_tile_lm<STRAT>(q, seg, pp, t - seg_first, ring + slot_off, ring_lds + 4u * slot_off, lane, acc,
                                       matched, la);
              }
              pslot = pslot + 1 == R ? 0 : pslot + 1;
              ++t;
            }
          } else {
            const bool nt = (rl(pp, 6) & kLmStreamNt) != 0;
            while (t < seg_end && ti < issue_end) {
              uint32_t slot_off = (uint32_t)(pslot * img_dw);
              if (nt)
                lm_wait_issue<true>(I, slot_off, R, D, ti - (t + 1), ring_lds + 4u * (uint32_t)(islot * img_dw),
                                    ti - ifirst, 16u * (uint32_t)lane);
              else
                lm_wait_issue(I, slot_off, R, D, ti - (t + 1), ring_lds + 4u * (uint32_t)(islot * img_dw), ti - ifirst,
                              16u * (uint32_t)lane);
              ++ti;
              islot = islot + 1 == R ? 0 : islot + 1;
              process_tile_lm<STRAT>(q, seg, pp, t - seg_first, ring + slot_off, ring_lds + 4u * slot_off, lane, acc,
                                     matched, la);
              pslot = pslot + 1 == R ? 0 : pslot + 1;
              ++t;
            }
          }
        }
      }
      for (; t < seg_end; ++t) {
        uint32_t slot_off = (uint32_t)(pslot * img_dw);
        wait_tile((int)(ti - (t + 1)), D, slot_off);  // tile t has landed in its slot (same-wave LDS-DMA)
        if (ti < t1) issue_next();                     // refill the slot tile t-1 used
        if (!stream_only) {
          if constexpr (LM) process_tile_lm<STRAT>(q, seg, pp, t - seg_first, ring + slot_off, ring_lds + 4u * slot_off, lane, acc, matched, la);
          else process_tile<STRAT, STEPS>(q, seg, t - seg_first, ring + slot_off, lane, acc, matched, la);
        }
        pslot = pslot + 1 == R ? 0 : pslot + 1;
      }
      if constexpr (is_lane(STRAT) && STRAT != STRAT_LANE_CNT) lane_acc_segment_end(q, seg, la, matched != matched_seg0);
      if constexpr (STRAT == STRAT_SELECT) sel_segment_docs(q, seg, matched, matched_seg0, lane);
      if (t < t1) {
        ++si;
        while (t >= segs[si].first_wtile + segs[si].num_wtiles) ++si;
      }
    }
  }

  if constexpr (!is_pcount(STRAT) && !is_pemit(STRAT))
    if (q->leap_mode) {
      // the entries kept in LDS to the wave's slice, then its count (every wave: the search kernel reads every count)
      const uint32_t nl = min(la.leap_n, (uint32_t)q->leap_lds_cap);
      AS1 unsigned long long* list = gp(q->leap_out) + 3 * (int64_t)q->num_segments + 1 + (int64_t)q->leap_slices +
                                     (int64_t)la.leap_slice * (int64_t)q->leap_cap;
      const lds_u64_t* ll = (const lds_u64_t*)(uintptr_t)la.leap_lds;
      for (uint32_t k = (uint32_t)lane; k < nl; k += kWave) list[k] = ll[k];
      if (lane == 0) gp(q->leap_out)[3 * (int64_t)q->num_segments + 1 + la.leap_slice] = la.leap_n;
    }
  if constexpr (STRAT == STRAT_SELECT) sel_counters_flush(q, la, lane);
  if constexpr (STRAT == STRAT_DISTINCT_LDS) distinct_lds_flush<WGS>(q, lds_acc);
  if constexpr (STRAT == STRAT_FILTERED_LDS) filtered_lds_flush<WGS>(q, lds_acc);
  if constexpr (STRAT == STRAT_EXPR_LDS) lds_acc_flush<WGS>(q, lds_acc);
  if constexpr (STRAT == STRAT_TROW_LDS) trow_lds_flush<WGS>(q, lds_acc);
  if constexpr (STRAT == STRAT_MOM_LDS) mom_lds_flush<WGS>(q, lds_acc);
  if constexpr (is_trow(STRAT)) {  // (the wide form's second launch sees the docs the first counted)
    if (q->trow_pass == 2) matched = 0;
  }
  if (!is_pemit(STRAT)) {  // (the partitioned count pass counts numDocsScanned; its emit pass sees the same docs)
    const int64_t wm = wave_sum_i64((int64_t)matched);
    if (lane == 0 && wm != 0) __hip_atomic_fetch_add(gp(q->matched_docs), (unsigned long long)wm, RLX);
    if constexpr (is_lane(STRAT)) {  // COUNT(*) of an aggregation-only query = the docs the filter kept
      if (lane == 0 && wm != 0) __hip_atomic_fetch_add(gp(q->count), (unsigned long long)wm, RLX);
      if constexpr (STRAT == STRAT_LANE_DICT) lane_hist_fold<WGS>(q, segs, lds_acc, la);
      if constexpr (STRAT != STRAT_LANE_CNT) lane_acc_flush(q, la, lane);
    }
  }
  if constexpr (is_pcount(STRAT)) pcount_store<WGS>(q, lds_acc, ps, lb);
  if constexpr (is_pemit(STRAT)) pemit_finish<WGS>(q, lds_acc, ps, lb);
  if (STRAT == STRAT_LDS) lds_acc_flush<WGS>(q, lds_acc);
}

}  // namespace pa
