// The lane-major direct scan for "one equality, rare survivors" specialised to one query shape, compiled at
// pa_query_prepare by hiprtc with the shape as macros (pa_jit.hip eqs_plan). It restates scan_kernel<STRAT_GLOBAL, 32, 1>
// (pa_scan.h) for the shape of its hoisted single-range loop: persistent waves, each walking a contiguous range of
// 2048-doc lane-major tiles of ONE staged column (the equality's) through a ring of wave-private LDS-DMA tile images
// behind counted vmcnt waits; per tile the word-wise equality prefilter (pa_eq_any.h) on the lane's stream words, and
// only where some lane answers the exact compare (pa_scan.h leaf_lm) and the survivor path. The column width is a
// constant: no switch on bit widths, no plan table read through readlane, the DMA of a tile is straight-line code.
// Self-contained (hiprtc's built-in HIP headers; pa_jit_abi.h is pasted in by build.py).
//
// The survivor path is per doc, as the planner takes this kernel only where survivors are rare (a dictionary of at
// least 4096 values behind the equality): every other filter clause (one DICT_RANGE each) is decoded from HBM for the
// docs the equality kept, the fused execution statistics' list gets the tile's E docs (pa_scan.h leap_tile), the group
// key is read from the group-by columns' streams in HBM (through the segment's remap), and COUNT / SUM go to the
// table-wide accumulators with device-scope atomics, a LONG sum as its exact (low 32 bits, high 32 bits) pair like
// Acc<STRAT_GLOBAL>. Integer adds only: the result does not depend on their order.
//
// Reference semantics: ScanBasedFilterOperator over a dictId range (SVScanDocIdIterator.java:203), AndDocIdIterator
// (later clauses only on candidate docs), DefaultGroupByExecutor.process (DefaultGroupByExecutor.java:131-158),
// DictionaryBasedGroupKeyGenerator raw keys, SumAggregationFunction.aggregateGroupBySV (:207), CountAggregationFunction.
//
// Shape macros (all integers; lists as {a, b, ...}):
//   JIT_W waves per workgroup, JIT_WG workgroups per CU the launch is planned for, JIT_RING tile images per wave,
//   JIT_IMG dwords of one tile image (the column's region starts at byte 16, behind a guard),
//   JIT_NCLS width classes (segments with their own dictionaries: at most 4), JIT_NB {bits of the column per class},
//   JIT_NT 1: the column DMAs carry the nt cache policy (as stream_nt for the generic kernel),
//   JIT_NLZ lazy DICT_RANGE clauses, JIT_NG group-by columns, JIT_NA SUM aggregations,
//   JIT_LEAP 1: the fused execution statistics (DevQuery::leap_mode),
//   JIT_DBG 1: measurement only (tuning eqs_dbg; results invalid): stream the tiles only
typedef unsigned int u32;
typedef unsigned long long u64;
typedef long long i64;
typedef __attribute__((address_space(3))) u32 l32;
typedef __attribute__((address_space(3))) u64 l64;
typedef const __attribute__((address_space(1))) u32 g32;
typedef const __attribute__((address_space(1))) int gi32;
typedef const __attribute__((address_space(1))) i64 gi64;
typedef __attribute__((address_space(1))) u64 gu64;

#include "pa_jit_abi.h"

#ifndef JIT_DBG
#define JIT_DBG 0
#endif
constexpr int W = JIT_W, R = JIT_RING, IMG = JIT_IMG, NCLS = JIT_NCLS, NLZ = JIT_NLZ, NG = JIT_NG, NA = JIT_NA;
constexpr int kNB[NCLS] = JIT_NB;
constexpr int TD = 2048;        // docs per tile: lane l holds docs [32 l, 32 l + 32), the column's words [l NB, (l + 1) NB)
constexpr u32 REG = 16;         // byte offset of the column's region in a tile image
static_assert(R >= 2 && R <= 8, "2..8 tile images per wave");
static_assert(NCLS >= 1 && NCLS <= 4, "1..4 width classes");
static_assert(NLZ <= kJitMax && NG <= kJitMaxGb && NA <= kJitMax, "shape beyond the JIT descriptors");

typedef const __attribute__((address_space(4))) JitArgs CA;
typedef const __attribute__((address_space(4))) EqsHdr CH;
typedef const __attribute__((address_space(4))) EqsSeg CS;

__device__ __forceinline__ u32 lds_addr(const void* p) { return (u32)(unsigned long)(const l32*)p; }
template <class T>
__device__ __forceinline__ T* at(u32 a) { return (T*)(unsigned long)a; }

template <int N>
__device__ __forceinline__ void vm_wait() {
  static_assert(N >= 0 && N < 64, "vmcnt is 6 bits");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// LDS-DMA with a scalar base: lane l copies 16 bytes at sbase + voff to dst + 16 l (mask: the taking-part lanes)
#if JIT_NT
#define EQS_MOD " nt"
#else
#define EQS_MOD ""
#endif
__device__ __forceinline__ void dma16(u32 voff, u64 sbase, u32 dst) {
  u32 keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" EQS_MOD
               "\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(dst));
}
__device__ __forceinline__ void dma16m(u32 voff, u64 sbase, u32 dst, u64 mask) {
  u32 keep;
  u64 save;
  asm volatile(
      "s_mov_b64 %1, exec\n\ts_mov_b64 exec, %5\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\t"
      "global_load_lds_dwordx4 %2, %3" EQS_MOD "\n\ts_mov_b32 m0, %0\n\ts_mov_b64 exec, %1"
      : "=&s"(keep), "=&s"(save) : "v"(voff), "s"(sbase), "s"(dst), "s"(mask));
}

// wave DMA instructions of one tile of an NB-bit column: 256 NB bytes as 16 NB chunks of 16 bytes, 64 per instruction
constexpr int dma_instrs(int nb) { return (16 * nb + 63) / 64; }
constexpr int dma_max() {
  int n = 0;
  for (int k = 0; k < NCLS; ++k) n = dma_instrs(kNB[k]) > n ? dma_instrs(kNB[k]) : n;
  return n;
}
// every tile is exactly D instructions, so that vmcnt counts tiles: classes of different widths pad with 16-byte
// copies into the image's guard (one class: no padding)
constexpr int D = dma_max();
static_assert((R - 2) * D < 64, "the counted wait must fit vmcnt");

template <int K>
__device__ __forceinline__ void dma_tile_k(u64 src, int wt, u32 img, u32 voff) {
  constexpr int NB = kNB[K];
  constexpr int CH = 16 * NB;
  const u64 s = src + (u64)(u32)wt * (u64)(256 * NB);
  const u32 dst = img + REG;
#pragma unroll
  for (int k = 0; k < CH / 64; ++k) dma16(voff, s + 1024u * k, dst + 1024u * k);
  if constexpr (CH % 64) dma16m(voff, s + 1024u * (CH / 64), dst + 1024u * (CH / 64), (1ull << (CH % 64)) - 1ull);
#pragma unroll
  for (int k = dma_instrs(NB); k < D; ++k) dma16m(voff, src, img, 1ull);
}
template <int K>
__device__ __forceinline__ void dma_tile(int cls, u64 src, int wt, u32 img, u32 voff) {
  if constexpr (K + 1 < NCLS) {
    if (cls == K) dma_tile_k<K>(src, wt, img, voff);
    else dma_tile<K + 1>(cls, src, wt, img, voff);
  } else {
    dma_tile_k<K>(src, wt, img, voff);
  }
}

// ---------------------------------------------------------------- the equality prefilter (pa_eq_any.h, one width)
// A lane's 32 docs are one string of 32 NB bits, word 0 first, every word MSB first. XOR with "every doc equals v" (the
// pattern words) makes a matching doc an all-zero field, and (x - L) & ~x & H != 0 <=> some field of x is zero, L / H
// the lowest / highest bit of every field; the subtraction runs from the last word to the first, borrow handed on.
template <int NB>
constexpr u32 eq_low_bits(int w) {
  u32 m = 0;
  for (int i = 0; i < 32; ++i) {
    const int s = (i + 1) * NB - 1;
    if ((s >> 5) == w) m |= 0x80000000u >> (s & 31);
  }
  return m;
}
template <int NB>
constexpr u32 eq_high_bits(int w) {
  u32 m = 0;
  for (int i = 0; i < 32; ++i) {
    const int s = i * NB;
    if ((s >> 5) == w) m |= 0x80000000u >> (s & 31);
  }
  return m;
}
// pattern word j: the 32 bits of the repetition from stream bit 32 j, i.e. from bit (32 j) % NB of a field
template <int NB>
__device__ __forceinline__ u32 eq_pattern_word(u64 window, int j) {
  return (u32)((window << ((32 * j) % NB)) >> 32);
}
template <int NB, int J>
__device__ __forceinline__ void eq_any_word(const u32 (&p)[NB], const u32 (&pat)[NB], u64& borrow, u32& any) {
  constexpr u32 L = eq_low_bits<NB>(J), H = eq_high_bits<NB>(J);
  const u32 x = p[J] ^ pat[J];
  u32 d;
  // d = x - L - borrow, borrow out; both operands in vector registers: the borrow's scalar pair is the one scalar
  // operand the instruction may read
  asm("v_subb_co_u32_e64 %[d], %[b], %[x], %[l], %[b]" : [d] "=v"(d), [b] "+s"(borrow) : [x] "v"(x), [l] "v"(L));
  any |= d & ~x & H;
  if constexpr (J > 0) eq_any_word<NB, J - 1>(p, pat, borrow, any);
}

// ---------------------------------------------------------------- the exact compare (pa_scan.h leaf_lm, DICT_RANGE)
// bit i <=> doc 32 lane + i matches: lo <= v < lo + span <=> (t - lo') <= hi' on the MSB-aligned value t; over the
// lane's words as the prefilter read them (the kernel has the registers to keep them all)
template <int NB>
__device__ __forceinline__ u32 leaf_eq(const u32 (&w)[NB], u32 lo_t, u32 hi_t) {
  u32 nm = 0;
#pragma unroll
  for (int i = 31; i >= 0; --i) {
    const int s = i * NB, j = s >> 5, o = s & 31;
    const u32 t = (o + NB <= 32) ? (w[j] << o) : __builtin_amdgcn_alignbit(w[j], w[j + 1 < NB ? j + 1 : j], 32 - o);
    u32 u;
    asm("v_sub_u32_e64 %[u], %[t], %[lo]\n\tv_sub_co_u32_e32 %[u], vcc, %[hi], %[u]\n\t"
        "v_addc_co_u32_e32 %[nm], vcc, %[nm], %[nm], vcc"
        : [nm] "+v"(nm), [u] "=&v"(u) : [t] "v"(t), [lo] "s"(lo_t), [hi] "s"(hi_t) : "vcc");
  }
  return ~nm;
}

// ---------------------------------------------------------------- the survivor path (rare)
// value of doc `doc` of an nb-bit stream in HBM (words[-1] is a guard word): pa_scan.h decode_global
__device__ __forceinline__ u32 decode_global(u64 words, i64 doc, int nb) {
  const u64 e1 = (u64)doc * (u64)nb + (u64)(nb - 1);
  const i64 we = (i64)(e1 >> 5);
  const u32 lo = ((g32*)words)[we];
  const u32 hi = ((g32*)words)[we - 1];
  return __builtin_amdgcn_alignbit(hi, lo, (~(u32)e1) & 31u) & (nb >= 32 ? 0xffffffffu : ((1u << nb) - 1u));
}

// The E docs of one tile (e: the equality's bits, f: those the other clauses kept too) into the wave's list slice, the
// tile's matched docs into the segment's counter (pa_scan.h leap_tile, lane-major; the layout of leap_out is there).
__device__ __forceinline__ u32 leap_tile(CH* Hd, int si, i64 doc_base, u32 e, u32 f, int lane, u32 slice, u32 listed,
                                         u32 lds_base) {
  const u32 mine = (u32)__builtin_popcount(e);
  u32 incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u32 t = (u32)__shfl_up((int)incl, o, 64);
    if (lane >= o) incl += t;
  }
  const u32 total = (u32)__builtin_amdgcn_readlane((int)incl, 63);
  u32 matched = (u32)__builtin_popcount(f);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) matched += (u32)__shfl_xor((int)matched, o, 64);
  const i64 nseg = Hd->nseg;
  const u64 cap = (u64)Hd->leap_cap;
  gu64* out = (gu64*)Hd->leap_out;
  if ((u64)listed + total > cap) {
    if (lane == 0) __hip_atomic_fetch_or(out + 3 * nseg, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    gu64* list = out + 3 * nseg + 1 + Hd->leap_slices + (i64)slice * (i64)cap;
    const u32 lcap = (u32)Hd->leap_lds_cap;
    u32 pos = listed + (incl - mine);
    while (e) {
      const int i = __builtin_ctz(e);
      e &= e - 1u;
      const i64 doc = doc_base + 32 * lane + i;
      const u64 ent = ((u64)si << 40) | ((u64)doc << 1) | ((f >> i) & 1u);
      if (pos < lcap) at<l64>(lds_base)[pos] = ent;
      else list[pos] = ent;
      ++pos;
    }
  }
  if (lane == 0 && matched)
    __hip_atomic_fetch_add(out + 3 * (i64)si, (u64)matched, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return listed + total;
}

struct Surv {
  u32 matched, listed;  // the lane's docs counted in numDocsScanned; the wave's list entries so far
};

// A tile where the equality kept some doc (m: the lane's 32 match bits): the other clauses per doc, then the group key
// and the accumulators per matching doc. Not inlined: the tile loop keeps its registers.
__device__ __noinline__ Surv survivors(CA* A, CH* Hd, CS* sg, i64 doc_base, u32 m, int lane, u32 slice, u32 listed,
                                       u32 leap_lds) {
  if constexpr (NLZ > 0) {
    const u32 eager = m;
#pragma unroll 1
    for (int i = 0; i < 32; ++i) {
      const u32 bit = 1u << i;
      if (__builtin_amdgcn_ballot_w64((m & bit) != 0) == 0) continue;
      const i64 doc = doc_base + 32 * lane + i;
      bool ok = (m & bit) != 0;
#pragma unroll
      for (int l = 0; l < NLZ; ++l) {
        if (ok) {
          const u32 id = decode_global(sg->lazy[l].words, doc, sg->lazy[l].nb);
          ok = ((id - sg->lazy[l].lo) < sg->lazy[l].span) != (sg->lazy[l].neg != 0);
        }
      }
      if (!ok) m &= ~bit;
    }
    if constexpr (JIT_LEAP) listed = leap_tile(Hd, sg->index, doc_base, eager, m, lane, slice, listed, leap_lds);
  }
  if (__builtin_amdgcn_ballot_w64(m != 0) != 0) {
#pragma unroll 1
    for (int i = 0; i < 32; ++i) {
      const u32 bit = 1u << i;
      if (__builtin_amdgcn_ballot_w64((m & bit) != 0) == 0) continue;
      if ((m & bit) == 0) continue;
      const i64 doc = doc_base + 32 * lane + i;
      // table-wide group key (DictionaryBasedGroupKeyGenerator: rawKey = sum dictId_j * prod_{k<j} card_k)
      i64 key = 0;
#pragma unroll
      for (int j = 0; j < NG; ++j) {
        u32 id = decode_global(sg->gb[j].words, doc, sg->gb[j].nb);
        if (sg->gb[j].tab != 0) id = (u32)((gi32*)sg->gb[j].tab)[id];
        key += (i64)((u64)id * (u64)Hd->gb_stride[j]);
      }
      __hip_atomic_fetch_add((gu64*)A->count + key, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        const u32 id = decode_global(sg->sum[a].words, doc, sg->sum[a].nb);
        const i64 v = ((gi64*)sg->sum[a].tab)[id];
        gu64* acc = (gu64*)A->sum[a];
        if (A->sum_long[a]) {  // exact (low 32 bits unsigned, high 32 bits signed) pair
          __hip_atomic_fetch_add(acc + 2 * key, (u64)(u32)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_fetch_add(acc + 2 * key + 1, (u64)(v >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
          __hip_atomic_fetch_add(acc + key, (u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
  }
  vm_wait<0>();  // nothing of this path left pending: the tile loop's counted waits count DMAs only
  return Surv{(u32)__builtin_popcount(m), listed};
}

__device__ __forceinline__ int find_segment(CS* segs, int nseg, int t) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].first_tile <= t) lo = mid;
    else hi = mid - 1;
  }
  while (t >= segs[lo].first_tile + segs[lo].num_tiles) ++lo;  // (segments without a tile)
  return lo;
}

// The wave's walk: tiles [t, t1) (the planner keeps the query's tiles below 2^31: 32-bit scalar compares); the issue
// cursor runs R - 1 tiles ahead and may be in a later segment.
struct Walk {
  CA* A;
  CH* Hd;
  CS* S;
  int t, t1, ti;
  int isi;              // issue cursor: segment, its tile range, stream, class
  int ifirst, iend;
  u64 isrc;
  int icls;
  u32 ring, voff;
  int slot;             // ring slot of tile t
  int lane;
  u32 slice, listed, leap_lds, matched;
};

__device__ __forceinline__ void issue(Walk& w, int to) {
  if (w.ti < w.t1) {
    while (w.ti >= w.iend) {
      ++w.isi;
      w.ifirst = (int)w.S[w.isi].first_tile;
      w.iend = w.ifirst + w.S[w.isi].num_tiles;
      w.isrc = w.S[w.isi].src;
      w.icls = w.S[w.isi].cls;
    }
    dma_tile<0>(w.icls, w.isrc, w.ti - w.ifirst, w.ring + (u32)to * (u32)(IMG * 4), w.voff);
  }
  ++w.ti;
}

// The tiles of segment `sg` (width class K) from w.t to `end`: every per-segment value is read here, once.
template <int K>
__device__ __forceinline__ void run(Walk& w, CS* sg, int end) {
  constexpr int NB = kNB[K];
  const int first = (int)sg->first_tile;
  const int full_end = first + sg->num_docs / TD;  // whole tiles; the ragged last one masks its padding
  const int num_docs = sg->num_docs;
  const u32 lo_t = sg->lo_t, hi_t = sg->hi_t;
  const u64 win = sg->win;
  u32 pat[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) pat[j] = eq_pattern_word<NB>(win, j);
  const u32 lane_words = REG + (u32)w.lane * (u32)(NB * 4);
  for (; w.t < end; ++w.t) {
    // tile t has landed: the R - 2 tiles after it may stay in flight when they were all issued
    if (R > 2 && w.t + (R - 2) < w.t1) vm_wait<(R > 2 ? (R - 2) * D : 0)>();
    else vm_wait<0>();
    issue(w, w.slot == 0 ? R - 1 : w.slot - 1);  // (into the image walked last)
    const u32 img = w.ring + (u32)w.slot * (u32)(IMG * 4);
    w.slot = w.slot + 1 == R ? 0 : w.slot + 1;
    if constexpr (JIT_DBG == 1) continue;
    const l32* p = at<const l32>(img + lane_words);
    u32 wv[NB];  // the lane's stream words, all reads issued before the first is used
#pragma unroll
    for (int j = 0; j < NB; ++j) wv[j] = p[j];
    u32 any = 0;
    u64 borrow = 0;
    eq_any_word<NB, NB - 1>(wv, pat, borrow, any);
    if (__builtin_amdgcn_ballot_w64(any != 0) == 0) continue;
    u32 m = leaf_eq<NB>(wv, lo_t, hi_t);
    if (w.t >= full_end) {  // the padding of a ragged tile is zero bits: it must not match dictId 0
      const i64 n = (i64)num_docs - (i64)(w.t - first) * TD - 32 * w.lane;
      m &= n >= 32 ? 0xffffffffu : (n <= 0 ? 0u : ((1u << n) - 1u));
    }
    if (__builtin_amdgcn_ballot_w64(m != 0) == 0) continue;
    const Surv s = survivors(w.A, w.Hd, sg, (i64)(w.t - first) * TD, m, w.lane, w.slice, w.listed, w.leap_lds);
    w.matched += s.matched;
    w.listed = (u32)__builtin_amdgcn_readfirstlane((int)s.listed);
  }
}
template <int K>
__device__ __forceinline__ void run_any(int cls, Walk& w, CS* sg, int end) {
  if constexpr (K + 1 < NCLS) {
    if (cls == K) run<K>(w, sg, end);
    else run_any<K + 1>(cls, w, sg, end);
  } else {
    run<K>(w, sg, end);
  }
}

extern "C" __global__ void __launch_bounds__(W * 64, JIT_WG) eqs_jit(const JitArgs* a_in, const EqsHdr* h_in) {
  CA* A = (CA*)(unsigned long)a_in;
  CH* Hd = (CH*)(unsigned long)h_in;
  CS* S = (CS*)(unsigned long)(h_in + 1);  // the segments follow the header
  extern __shared__ __attribute__((aligned(16))) u32 smem[];
  const u32 base = lds_addr(smem);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const i64 T = A->total_tiles, G = gridDim.x;
  const i64 b = blockIdx.x;
  const i64 lb = A->xcd_major ? (b % 8) * (G / 8) + (b % 8 < G % 8 ? b % 8 : G % 8) + b / 8 : b;
  const i64 gw = lb * W + wave, NW = G * W;
  Walk w;
  w.A = A;
  w.Hd = Hd;
  w.S = S;
  w.t = (int)(gw * T / NW);
  w.t1 = (int)((gw + 1) * T / NW);
  w.lane = lane;
  w.ring = base + (u32)wave * (u32)(R * IMG * 4);
  w.voff = 16u * (u32)lane;
  w.slot = 0;
  w.slice = (u32)gw;
  w.listed = 0;
  w.matched = 0;
  w.leap_lds = base + (u32)(W * R * IMG * 4) + (u32)wave * (u32)Hd->leap_lds_cap * 8u;
  if (w.t < w.t1) {
    const int nseg = A->nseg;
    int si = find_segment(S, nseg, w.t);
    w.isi = si;
    w.ifirst = (int)S[si].first_tile;
    w.iend = w.ifirst + S[si].num_tiles;
    w.isrc = S[si].src;
    w.icls = S[si].cls;
    w.ti = w.t;
#pragma unroll
    for (int k = 0; k + 1 < R; ++k) issue(w, k);
    while (w.t < w.t1) {
      CS* sg = S + si;
      const int seg_end = (int)sg->first_tile + sg->num_tiles;
      run_any<0>(sg->cls, w, sg, seg_end < w.t1 ? seg_end : w.t1);
      if (w.t < w.t1) {
        ++si;
        while (w.t >= S[si].first_tile + S[si].num_tiles) ++si;
      }
    }
    vm_wait<0>();
  }
  if constexpr (JIT_LEAP) {
    // the entries kept in LDS to the wave's slice, then its count (every wave: the search kernel reads every count)
    gu64* out = (gu64*)Hd->leap_out;
    const i64 nseg = Hd->nseg;
    const u32 lcap = (u32)Hd->leap_lds_cap;
    const u32 nl = w.listed < lcap ? w.listed : lcap;
    gu64* list = out + 3 * nseg + 1 + Hd->leap_slices + (i64)w.slice * Hd->leap_cap;
    for (u32 k = (u32)lane; k < nl; k += 64) list[k] = at<const l64>(w.leap_lds)[k];
    if (lane == 0) out[3 * nseg + 1 + w.slice] = w.listed;
  }
  u64 wm = w.matched;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) wm += __shfl_xor(wm, o);
  if (lane == 0 && wm) __hip_atomic_fetch_add((gu64*)A->matched, wm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
