// Scan strategy: aggregation-only queries, per-lane accumulators (the STRAT_LANE family).
// Included by the pa_scan_lane_*.hip units in place of pa_scan.h, which declares the entry points it calls and includes no strategy.
#pragma once
#include "pa_scan.h"

namespace pa {

// ---------------------------------------------------------------- aggregation-only queries (STRAT_LANE)
// Every lane keeps its own running SUM / MIN / MAX of aggregation a in (r0[a], r1[a]) for the whole kernel (COUNT is the
// filter's own doc count): SUM over int32 values r0 += v; over 64-bit values the exact split pair r0 += low 32 bits
// (unsigned), r1 += v >> 32 (a 96-bit total, like PA_ACC_SUM_I64X2); over FLOAT/DOUBLE r0 holds the bits of a double
// sum; MIN / MAX r0 = running min / max (doubles in the order-preserving encoding). The wave reduces them once, at the
// end of the kernel (lane_acc_flush). Reference: AggregationOperator -> SumAggregationFunction.aggregate (a running sum
// over the block's values), Min/MaxAggregationFunction.aggregate.
// MIN / MAX over a sorted dictionary run on dictIds (rid[a]: the lane's min / max dictId within the current segment),
// folded into r0 as a value at the end of every segment run (lane_acc_segment_end).
typedef __attribute__((address_space(3))) int64_t lds_i64_t;
__device__ __forceinline__ void la_get(const WaveState& la, int a, int64_t& r0, int64_t& r1) {
  const lds_i64_t* p = (const lds_i64_t*)(uintptr_t)(la.pair + (uint32_t)a * la.astr);
  r0 = p[0];
  r1 = p[1];
}
__device__ __forceinline__ void la_set(const WaveState& la, int a, int64_t r0, int64_t r1) {
  lds_i64_t* p = (lds_i64_t*)(uintptr_t)(la.pair + (uint32_t)a * la.astr);
  p[0] = r0;
  p[1] = r1;
}
__device__ __forceinline__ uint32_t la_rid(const WaveState& la, int a) {
  return *(const lds_u32_t*)(uintptr_t)(la.id + (uint32_t)a * (la.astr >> 2));
}
__device__ __forceinline__ void la_set_rid(const WaveState& la, int a, uint32_t v) {
  *(lds_u32_t*)(uintptr_t)(la.id + (uint32_t)a * (la.astr >> 2)) = v;
}

__device__ __forceinline__ uint32_t rid_init(int t) { return t == PA_AGG_MIN ? 0xffffffffu : 0u; }

__device__ __forceinline__ void lane_acc_init(const DevQuery* __restrict__ q, WaveState& la, const void* lds_area,
                                              int wgs) {
  la.astr = 16u * (uint32_t)wgs;
  la.pair = lds_addr(lds_area) + 16u * threadIdx.x;
  la.id = lds_addr(lds_area) + (uint32_t)q->num_aggs * la.astr + 4u * threadIdx.x;
  la.idm = 0;
  for (int a = 0; a < q->num_aggs && a < kLaneAggs; ++a) {
    const int t = q->aggs[a].type;
    la_set(la, a, t == PA_AGG_MIN ? INT64_MAX : (t == PA_AGG_MAX ? INT64_MIN : 0), 0);
    la_set_rid(la, a, rid_init(t));
  }
}

// Lane-major fast path modes (lane_agg_lm)
enum LaneMode : int { LM_SUM_INT = 0, LM_SUM_LONG = 1, LM_SUM_DOUBLE = 2, LM_MIN_ID = 3, LM_MAX_ID = 4 };

// One aggregation over the 32 docs of this lane in a lane-major tile (docs 32*lane + i, match bit i of m) from a staged
// dictionary column of NB-bit ids: the lane's NB stream words are read once and every id is a constant-shift extract.
// SUM: the value is a buffer load of dict[id] with a buffer resource bounded by the dictionary, and a doc that does not
// match asks for index 0xffffffff (its bit of ~m spread by a signed bitfield extract, ORed into the id): out of range,
// so the load returns 0 — no per-doc branch or select. MIN_ID / MAX_ID track the smallest / largest matching dictId
// (0xffffffff is neutral under unsigned min; a non-matching id is ANDed to 0 for max).
template <int NB>
__device__ __forceinline__ void lane_agg_lm(uint32_t region_lds, int lane, uint32_t m, int mode,
                                            __amdgpu_buffer_rsrc_t dict, int64_t& r0, int64_t& r1, uint32_t& rid) {
  const lds_u32_t* p = (const lds_u32_t*)(uintptr_t)(region_lds + (uint32_t)lane * (uint32_t)(NB * 4));
  constexpr int H = NB > 16 ? 2 : 1;  // halves of 16 docs for wide columns (live stream words stay ~NB/2 + 1)
  constexpr int DPH = 32 / H;
  const uint32_t nm = ~m;
#pragma unroll
  for (int h = 0; h < H; ++h) {
    constexpr int WMAX = (DPH * NB + 31) / 32 + 1;
    const int wlo = (h * DPH * NB) >> 5;
    uint32_t w[WMAX];
#pragma unroll
    for (int j = 0; j < WMAX; ++j) w[j] = (wlo + j < NB) ? p[wlo + j] : 0u;
    auto id_of = [&](int i) -> uint32_t {
      const int s = i * NB, j = (s >> 5) - wlo, o = s & 31;
      if (o + NB <= 32) return __builtin_amdgcn_ubfe(w[j], (uint32_t)(32 - o - NB), (uint32_t)NB);
      return __builtin_amdgcn_alignbit(w[j], w[(j + 1 < WMAX) ? j + 1 : j], 32 - o) >> (32 - NB);
    };
    if (mode <= LM_SUM_DOUBLE) {
      uint64_t v[DPH];
#pragma unroll
      for (int k = 0; k < DPH; ++k) {
        const int i = h * DPH + k;
        const uint32_t off = (id_of(i) << 3) | (uint32_t)__builtin_amdgcn_sbfe((int)nm, (uint32_t)i, 1u);
        v[k] = __builtin_bit_cast(uint64_t, __builtin_amdgcn_raw_buffer_load_b64(dict, off, 0, 0));
      }
      if (mode == LM_SUM_INT) {
#pragma unroll
        for (int k = 0; k < DPH; ++k) r0 += (int64_t)v[k];
      } else if (mode == LM_SUM_LONG) {
#pragma unroll
        for (int k = 0; k < DPH; ++k) {
          r0 += (int64_t)(uint32_t)v[k];
          r1 += (int64_t)v[k] >> 32;
        }
      } else {
        double d = __builtin_bit_cast(double, r0);
#pragma unroll
        for (int k = 0; k < DPH; ++k) d += __builtin_bit_cast(double, v[k]);
        r0 = __builtin_bit_cast(int64_t, d);
      }
    } else if (mode == LM_MIN_ID) {
#pragma unroll
      for (int k = 0; k < DPH; ++k) {
        const int i = h * DPH + k;
        rid = min(rid, id_of(i) | (uint32_t)__builtin_amdgcn_sbfe((int)nm, (uint32_t)i, 1u));
      }
    } else {
#pragma unroll
      for (int k = 0; k < DPH; ++k) {
        const int i = h * DPH + k;
        rid = max(rid, id_of(i) & (uint32_t)__builtin_amdgcn_sbfe((int)m, (uint32_t)i, 1u));
      }
    }
  }
}

__device__ __noinline__ void lane_agg_lm_any(int nb, uint32_t region_lds, int lane, uint32_t m, int mode,
                                                __amdgpu_buffer_rsrc_t dict, int64_t& r0, int64_t& r1, uint32_t& rid) {
  switch (nb) {
#define PA_LA_CASE(N) \
  case N: lane_agg_lm<N>(region_lds, lane, m, mode, dict, r0, r1, rid); break;
    PA_LA_CASE(1) PA_LA_CASE(2) PA_LA_CASE(3) PA_LA_CASE(4) PA_LA_CASE(5) PA_LA_CASE(6) PA_LA_CASE(7) PA_LA_CASE(8)
    PA_LA_CASE(9) PA_LA_CASE(10) PA_LA_CASE(11) PA_LA_CASE(12) PA_LA_CASE(13) PA_LA_CASE(14) PA_LA_CASE(15)
    PA_LA_CASE(16) PA_LA_CASE(17) PA_LA_CASE(18) PA_LA_CASE(19) PA_LA_CASE(20) PA_LA_CASE(21) PA_LA_CASE(22)
    PA_LA_CASE(23) PA_LA_CASE(24) PA_LA_CASE(25) PA_LA_CASE(26) PA_LA_CASE(27) PA_LA_CASE(28) PA_LA_CASE(29)
    PA_LA_CASE(30) PA_LA_CASE(31)
#undef PA_LA_CASE
    default: break;
  }
}

// End of a wave's run over one segment: MIN / MAX dictIds of the segment -> values, folded into r0 (only when the
// lane kept some doc of the segment: a MAX dictId of 0 is otherwise meaningless).
__device__ __forceinline__ void lane_acc_segment_end(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                                     WaveState& la, bool any) {
#pragma unroll
  for (int a = 0; a < kLaneAggs; ++a) {
    if (a >= q->num_aggs) break;
    const int t = q->aggs[a].type;
    if (t != PA_AGG_MIN && t != PA_AGG_MAX) continue;
    const uint32_t id = la_rid(la, a);
    la_set_rid(la, a, rid_init(t));
    if (!((la.idm >> a) & 1u) || !any || (t == PA_AGG_MIN && id == 0xffffffffu)) continue;
    const DevCol& c = seg->cols[q->aggs[a].slot];
    const int64_t e = q->aggs[a].src == SRC_DOUBLE ? f64_order_encode(gp(c.dict_f64)[id]) : gp(c.dict_i64)[id];
    int64_t r0, r1;
    la_get(la, a, r0, r1);
    la_set(la, a, t == PA_AGG_MIN ? (e < r0 ? e : r0) : (e > r0 ? e : r0), r1);
  }
  la.idm = 0;
}

// One value (int64, or double bits for SRC_DOUBLE) into a lane accumulator pair: SUM over int32-range values r0 += v;
// 64-bit integer SUM as the exact split pair (r0 += low 32 bits unsigned, r1 += high 32 bits signed); double SUM in
// r0's bits; MIN / MAX on the order-preserving encoding.
__device__ __forceinline__ void lane_fold(int type, int src, uint64_t v, int64_t& r0, int64_t& r1) {
  if (type == PA_AGG_SUM) {
    if (src == SRC_INT) {
      r0 += (int64_t)v;
    } else if (src == SRC_LONG) {
      r0 += (int64_t)(uint32_t)v;
      r1 += (int64_t)v >> 32;
    } else {
      r0 = __builtin_bit_cast(int64_t, __builtin_bit_cast(double, r0) + __builtin_bit_cast(double, v));
    }
  } else {
    const int64_t e = src == SRC_DOUBLE ? f64_order_encode(__builtin_bit_cast(double, v)) : (int64_t)v;
    r0 = type == PA_AGG_MIN ? (e < r0 ? e : r0) : (e > r0 ? e : r0);
  }
}

// A raw value as the 64-bit pattern lane_fold takes: INT sign-extended, FLOAT widened to double bits, LONG / DOUBLE as is.
__device__ __forceinline__ uint64_t raw_bits(int vtype, uint64_t x) {
  switch (vtype) {
    case PA_INT: return (uint64_t)(int64_t)(int32_t)(uint32_t)x;
    case PA_FLOAT: return __builtin_bit_cast(uint64_t, (double)__builtin_bit_cast(float, (uint32_t)x));
    default: return x;
  }
}

// Sparse lane-major tile (few matching docs): each lane walks its own set bits of m (doc 32*lane + i), four per batch so
// their loads overlap; the wave loops max-popcount times instead of over all 32 docs. `load(i)` issues the value load of
// doc i (nothing is consumed before all four are issued).
template <class LOAD>
__device__ __forceinline__ void lane_sparse(uint32_t m, int type, int src, LOAD load, int64_t& r0, int64_t& r1) {
  while (__ballot(m != 0) != 0) {
    bool on[4];
    uint64_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      on[k] = m != 0;
      const int i = on[k] ? __builtin_ctz(m) : 0;
      m &= m - 1u;
      v[k] = on[k] ? load(i) : 0ull;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (on[k]) lane_fold(type, src, v[k], r0, r1);
  }
}

// lane_sparse for a dictId histogram: every matching doc adds one to hist[dictId] (dec(i) = dictId of doc i); the
// decodes of a batch of four are issued before their (non-returning) LDS adds.
template <class DEC>
__device__ __forceinline__ void lane_sparse_hist(uint32_t m, DEC dec, lds_u32_t* hist) {
  while (__ballot(m != 0) != 0) {
    bool on[4];
    uint32_t id[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      on[k] = m != 0;
      const int i = on[k] ? __builtin_ctz(m) : 0;
      m &= m - 1u;
      id[k] = on[k] ? dec(i) : 0u;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (on[k]) __hip_atomic_fetch_add(hist + id[k], 1u, WG_RLX);
  }
}

// lane_sparse for MIN / MAX of a sorted dictionary: the smallest / largest matching dictId (dec(i) = dictId of doc i).
template <class DEC>
__device__ __forceinline__ void lane_sparse_ids(uint32_t m, bool is_min, DEC dec, uint32_t& rid) {
  while (__ballot(m != 0) != 0) {
    bool on[4];
    uint32_t id[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      on[k] = m != 0;
      const int i = on[k] ? __builtin_ctz(m) : 0;
      m &= m - 1u;
      id[k] = on[k] ? dec(i) : 0u;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (on[k]) rid = is_min ? min(rid, id[k]) : max(rid, id[k]);
  }
}

// Dense lane-major tile of a raw column of VB-byte values: the whole tile's values as coalesced 16-byte loads
// (instruction k, lane l: docs VPL*(64k + l) .. + VPL-1 of the tile, VPL = 16 / VB), every value's match bit read from
// the lane owning its doc in the lane-major layout (doc d: lane d >> 5, bit d & 31) by one ds_bpermute per
// instruction. Non-matching values are skipped by a select (no per-doc branch). Raw columns are padded to whole wave
// tiles, so the last tile's loads stay in bounds. 32 VGPRs of loads per batch, all issued before use.
template <int VB>
__device__ __forceinline__ void lane_raw_dense(const char* tile, uint32_t m, int lane, int vtype, int type, int src,
                                               int64_t& r0, int64_t& r1) {
  constexpr int VPL = 16 / VB;        // values per lane per instruction
  constexpr int NI = 2048 * VB / 1024;  // instructions per tile
  constexpr int KB = VB == 8 ? 4 : 8;
  const AS1 u32x4* p = (const AS1 u32x4*)tile + lane;
#pragma unroll
  for (int k0 = 0; k0 < NI; k0 += KB) {
    u32x4 w[KB];
    uint32_t mb[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      w[k] = p[(k0 + k) * kWave];
      // owner of doc VPL*(64k + l): lane 2*VPL*k + (VPL*l >> 5); its bits VPL*l & 31 .. + VPL-1
      const int owner = 2 * VPL * (k0 + k) + ((VPL * lane) >> 5);
      mb[k] = (uint32_t)__builtin_amdgcn_ds_bpermute(owner << 2, (int)m) >> ((VPL * lane) & 31);
    }
#pragma unroll
    for (int k = 0; k < KB; ++k) {
#pragma unroll
      for (int j = 0; j < VPL; ++j) {
        const uint64_t x = VB == 8 ? ((uint64_t)w[k][2 * j + 1] << 32) | w[k][2 * j] : (uint64_t)w[k][j];
        const bool on = (mb[k] >> j) & 1u;
        if (type == PA_AGG_SUM) {
          lane_fold(type, src, on ? raw_bits(vtype, x) : 0ull, r0, r1);  // (+0 / +0.0 for a doc that does not match)
        } else if (on) {
          lane_fold(type, src, raw_bits(vtype, x), r0, r1);
        }
      }
    }
  }
}

// The matching docs (match words m) of one tile into the lane accumulators: per aggregation, 8 steps per batch — every
// value load of the batch is issued before any is used (staged dictIds from the tile image, lazy ones and raw values from
// HBM, then the dictionary gathers).
template <int LM, int STEPS, int STRAT>
__device__ __forceinline__ void lane_acc_tile(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                              const uint32_t* img, int64_t doc_base, uint32_t m, int lane,
                                              WaveState& la, unsigned char* lds) {
  typedef const __attribute__((address_space(4))) DevSeg CSeg;
  CSeg* cs = (CSeg*)(uintptr_t)seg;
  auto local = [&](int i) { return LM ? 32 * lane + i : i * kWave + lane; };
  constexpr int kB = 8;
  const int na = q->num_aggs;
  // matching docs of the tile: the wave's total and the largest count of one lane (sparse vs dense paths)
  uint32_t tot = 0, mx = 0;
  if constexpr (LM) {
    tot = mx = (uint32_t)__builtin_popcount(m);
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      tot += (uint32_t)__shfl_xor((int)tot, o, kWave);
      mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, kWave));
    }
    tot = (uint32_t)__builtin_amdgcn_readfirstlane((int)tot);
    mx = (uint32_t)__builtin_amdgcn_readfirstlane((int)mx);
  }
  // one copy of the per-aggregation code (a loop that is not unrolled; the accumulators live in LDS): the unrolled form
  // replicated every path per aggregation and spilled
#pragma unroll 1
  for (int a = 0; a < na && a < kLaneAggs; ++a) {
    const int type = q->aggs[a].type;
    if (type == PA_AGG_COUNT) continue;
    const int slot = q->aggs[a].slot, src = q->aggs[a].src;
    const int kind = cs->cols[slot].kind, vtype = cs->cols[slot].vtype;
    const int loff = cs->cols[slot].lds_off, nb = cs->cols[slot].nbits;
    const uint32_t* words = cs->cols[slot].words;
    const uint64_t* dict = src == SRC_DOUBLE ? (const uint64_t*)cs->cols[slot].dict_f64
                                             : (const uint64_t*)cs->cols[slot].dict_i64;
    const void* raw = cs->cols[slot].raw;
    int64_t r0, r1;
    la_get(la, a, r0, r1);
    uint32_t rid = la_rid(la, a);
    do {  // (break: this aggregation is done)
    if (STRAT == STRAT_LANE_DICT) {
    } else if (LM && kind == COL_SV_RAW) {
      // raw column: per-doc loads of the few matching docs, or the whole tile as coalesced 16-byte loads (a sparse
      // tile's loads touch at most `tot` lines; the dense read is 2048 * VB bytes = 16 * VB lines of 128 B)
      const int vb = (vtype == PA_INT || vtype == PA_FLOAT) ? 4 : 8;
      if (tot <= (uint32_t)(6 * vb)) {
        const int64_t d0 = doc_base + 32 * lane;
        if (vb == 4) {
          const AS1 uint32_t* rp = gp((const uint32_t*)raw) + d0;
          lane_sparse(m, type, src, [&](int i) { return raw_bits(vtype, rp[i]); }, r0, r1);
        } else {
          const AS1 uint64_t* rp = gp((const uint64_t*)raw) + d0;
          lane_sparse(m, type, src, [&](int i) { return rp[i]; }, r0, r1);
        }
      } else if (vb == 4) {
        lane_raw_dense<4>((const char*)raw + doc_base * 4, m, lane, vtype, type, src, r0, r1);
      } else {
        lane_raw_dense<8>((const char*)raw + doc_base * 8, m, lane, vtype, type, src, r0, r1);
      }
      break;
    }
    if (STRAT == STRAT_LANE_RAW) break;  // (the raw kernel's columns are all raw: handled above)
    if constexpr (STRAT == STRAT_LANE_DICT) {
      if (type == PA_AGG_SUM && q->aggs[a].hist_card > 0) {
        // shared dictionary: count the dictIds in the workgroup's LDS histogram (the values come in at the end)
        lds_u32_t* hist = lds_ptr(lds + q->aggs[a].hist_off);
        lane_sparse_hist(m, [&](int i) -> uint32_t {
          return loff >= 0 ? decode_lds(img + loff, 32 * lane + i, nb) : decode_global(words, doc_base + 32 * lane + i, nb);
        }, hist);
        break;
      }
      // dictionary kernel: every tile walks the lanes' set bits (a lane's matching docs one after another, the wave
      // max-popcount times): decode from the staged image (or HBM when lazy), then MIN / MAX of a sorted dictionary on
      // the dictIds, anything else on the gathered values. One path (no per-width unpack calls): nothing spills.
      auto dec = [&](int i) -> uint32_t {
        return loff >= 0 ? decode_lds(img + loff, 32 * lane + i, nb) : decode_global(words, doc_base + 32 * lane + i, nb);
      };
      if (type != PA_AGG_SUM && (cs->cols[slot].flags & COLF_DICT_SORTED)) {
        lane_sparse_ids(m, type == PA_AGG_MIN, dec, rid);
        la.idm |= 1u << a;
      } else {
        lane_sparse(m, type, src, [&](int i) { return gp(dict)[dec(i)]; }, r0, r1);
      }
      break;
    }
    if (LM && kind == COL_SV_DICT && mx <= 12 &&
        !(type != PA_AGG_SUM && (cs->cols[slot].flags & COLF_DICT_SORTED) && loff >= 0)) {
      // dictionary column, few matching docs per lane: decode only those (staged image or HBM) and gather their values
      if (loff >= 0) {
        const uint32_t* region = img + loff;
        lane_sparse(m, type, src, [&](int i) { return gp(dict)[decode_lds(region, 32 * lane + i, nb)]; }, r0, r1);
      } else {
        const int64_t d0 = doc_base + 32 * lane;
        lane_sparse(m, type, src, [&](int i) { return gp(dict)[decode_global(words, d0 + i, nb)]; }, r0, r1);
      }
      break;
    }
    // (lane_agg_lm's 32-bit byte offset id << 3 and the resource's card * 8 bytes hold for dictionaries below 2^28
    // values; a larger one takes the generic gather below)
    if (LM && kind == COL_SV_DICT && loff >= 0 && cs->cols[slot].card < (1 << 28) &&
        (type == PA_AGG_SUM || (cs->cols[slot].flags & COLF_DICT_SORTED))) {
      const int mode = type == PA_AGG_SUM ? (src == SRC_INT ? LM_SUM_INT : (src == SRC_LONG ? LM_SUM_LONG : LM_SUM_DOUBLE))
                                          : (type == PA_AGG_MIN ? LM_MIN_ID : LM_MAX_ID);
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
          (void*)dict, (short)0, cs->cols[slot].card * 8, 0x00020000);
      lane_agg_lm_any(nb, lds_addr(img + loff), lane, m, mode, rs, r0, r1, rid);
      if (mode >= LM_MIN_ID) la.idm |= 1u << a;
      break;
    }
#pragma unroll 1
    for (int h = 0; h < STEPS; h += kB) {
      if (__ballot(((m >> h) & 0xffu) != 0) == 0) continue;
      uint64_t v[kB];
      if (kind == COL_SV_DICT) {
        uint32_t id[kB];
        decode_batch<kB, LM>(loff, nb, words, img, doc_base, h, m, lane, id);
#pragma unroll
        for (int i = 0; i < kB; ++i) v[i] = ((m >> (h + i)) & 1u) ? gp(dict)[id[i]] : 0ull;
      } else if (vtype == PA_INT) {
#pragma unroll
        for (int i = 0; i < kB; ++i)
          v[i] = ((m >> (h + i)) & 1u) ? (uint64_t)(int64_t)gp((const int32_t*)raw)[doc_base + local(h + i)] : 0ull;
      } else if (vtype == PA_FLOAT) {
#pragma unroll
        for (int i = 0; i < kB; ++i)
          v[i] = ((m >> (h + i)) & 1u) ? __builtin_bit_cast(uint64_t, (double)gp((const float*)raw)[doc_base + local(h + i)])
                                      : 0ull;
      } else {  // LONG, DOUBLE bits
#pragma unroll
        for (int i = 0; i < kB; ++i)
          v[i] = ((m >> (h + i)) & 1u) ? gp((const uint64_t*)raw)[doc_base + local(h + i)] : 0ull;
      }
      if (type == PA_AGG_SUM) {
        if (src == SRC_INT) {
#pragma unroll
          for (int i = 0; i < kB; ++i) r0 += (int64_t)v[i];
        } else if (src == SRC_LONG) {
#pragma unroll
          for (int i = 0; i < kB; ++i) {
            r0 += (int64_t)(uint32_t)v[i];
            r1 += (int64_t)v[i] >> 32;
          }
        } else {
          double d = __builtin_bit_cast(double, r0);
#pragma unroll
          for (int i = 0; i < kB; ++i) d += __builtin_bit_cast(double, v[i]);  // (0.0 for the docs that do not match)
          r0 = __builtin_bit_cast(int64_t, d);
        }
      } else {
#pragma unroll
        for (int i = 0; i < kB; ++i) {
          if (!((m >> (h + i)) & 1u)) continue;
          const int64_t e = src == SRC_DOUBLE ? f64_order_encode(__builtin_bit_cast(double, v[i])) : (int64_t)v[i];
          r0 = type == PA_AGG_MIN ? (e < r0 ? e : r0) : (e > r0 ? e : r0);
        }
      }
    }
    } while (false);
    la_set(la, a, r0, r1);
    la_set_rid(la, a, rid);
  }
}

// End of the kernel: one wave reduction per accumulator and one device-scope atomic per wave.
__device__ __forceinline__ void lane_acc_flush(const DevQuery* __restrict__ q, const WaveState& la, int lane) {
#pragma unroll
  for (int a = 0; a < kLaneAggs; ++a) {
    if (a >= q->num_aggs) break;
    const DevAgg& A = q->aggs[a];
    if (A.type == PA_AGG_COUNT) continue;
    int64_t r0, r1;
    la_get(la, a, r0, r1);
    if (A.type == PA_AGG_SUM) {
      if (A.src == SRC_DOUBLE) {
        const double s = wave_sum_f64(__builtin_bit_cast(double, r0));
        if (lane == 0) __hip_atomic_fetch_add(gp(A.acc_f64), s, RLX);
      } else if (A.src == SRC_LONG) {
        const int64_t lo = wave_sum_i64(r0), hi = wave_sum_i64(r1);
        if (lane == 0) {
          __hip_atomic_fetch_add(gp((unsigned long long*)A.acc_i64), (unsigned long long)lo, RLX);
          __hip_atomic_fetch_add(gp((unsigned long long*)A.acc_i64) + 1, (unsigned long long)hi, RLX);
        }
      } else {
        const int64_t s = wave_sum_i64(r0);
        if (lane == 0) __hip_atomic_fetch_add(gp((unsigned long long*)A.acc_i64), (unsigned long long)s, RLX);
      }
    } else if (A.type == PA_AGG_MIN) {
      const int64_t r = wave_min_i64(r0);
      if (lane == 0 && r != INT64_MAX) __hip_atomic_fetch_min(gp((long long*)A.acc_i64), (long long)r, RLX);
    } else {
      const int64_t r = wave_max_i64(r0);
      if (lane == 0 && r != INT64_MIN) __hip_atomic_fetch_max(gp((long long*)A.acc_i64), (long long)r, RLX);
    }
  }
}

// STRAT_LANE_DICT, start of the kernel: the dictId histograms of SUMs over a shared dictionary to zero.
template <int WGS>
__device__ __forceinline__ void lane_hist_zero(const DevQuery* q, unsigned char* lds_acc) {
  for (int a = 0; a < q->num_aggs; ++a) {
    const int hc = q->aggs[a].hist_card;
    if (hc <= 0) continue;
    uint32_t* h = (uint32_t*)(lds_acc + q->aggs[a].hist_off);
    for (int i = threadIdx.x; i < hc; i += WGS) h[i] = 0u;
  }
  __syncthreads();
}

// STRAT_LANE_DICT, end of the kernel, before lane_acc_flush.
template <int WGS>
__device__ __forceinline__ void lane_hist_fold(const DevQuery* q, const DevSeg* segs, unsigned char* lds_acc,
                                               const WaveState& la) {
  // each thread folds histogram entries t, t + WGS, ... : count * value into its lane accumulator (exact split
  // pair for 64-bit values: count < 2^32, so count * low32 and count * high32 fit their int64 halves)
  __syncthreads();
  for (int a = 0; a < q->num_aggs; ++a) {
    const DevAgg& A = q->aggs[a];
    if (A.hist_card <= 0) continue;
    const uint32_t* h = (const uint32_t*)(lds_acc + A.hist_off);
    const DevCol& c = segs[0].cols[A.slot];
    int64_t r0, r1;
    la_get(la, a, r0, r1);
    for (int i = threadIdx.x; i < A.hist_card; i += WGS) {
      const uint32_t n = h[i];
      if (n == 0) continue;
      if (A.src == SRC_DOUBLE) {
        r0 = __builtin_bit_cast(int64_t, __builtin_bit_cast(double, r0) + (double)n * gp(c.dict_f64)[i]);
      } else {
        const int64_t v = gp(c.dict_i64)[i];
        if (A.src == SRC_INT) {
          r0 += (int64_t)n * v;
        } else {
          r0 += (int64_t)n * (int64_t)(uint32_t)v;
          r1 += (int64_t)n * (v >> 32);
        }
      }
    }
    la_set(la, a, r0, r1);
  }
}

}  // namespace pa
