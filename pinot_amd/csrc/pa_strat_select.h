// Scan strategy: selection (STRAT_SELECT), with the entry order and threshold search of pa_select.hip.
// Included by pa_scan_select.hip and pa_select.hip in place of pa_scan.h, which declares the entry points it calls and includes no strategy.
#pragma once
#include "pa_scan.h"

namespace pa {

// ---------------------------------------------------------------- selection (STRAT_SELECT)
// SELECT ... ORDER BY ... LIMIT: the scan keeps, per wave, the candidates for the K smallest (key, row) entries of the
// docs the filter kept (SelectionOrderByOperator.java:139-188: every matching doc offered to a bounded priority queue).
// A wave owns a segment of CAP > K entries in an HBM scratch block and a private bound (its K-th smallest entry so far,
// all ones at first): an entry below the bound is appended; a full segment is compacted in place to its K smallest
// entries by a radix select over the 128-bit entries (linear, no sort), whose K-th becomes the bound. After a compaction
// the wave publishes its K-th KEY to one global word (relaxed atomic min); every wave reads that word once per tile with
// survivors and drops entries whose key exceeds it (inclusive: the row part is unknown; a stale read is only a looser
// bound, so nothing is ordered). All candidate state is wave-private: no workgroup barrier in the tile loop (the waves
// of a workgroup own tile ranges of different lengths). The finish kernels (pa_select.hip) select and sort the K
// smallest of all waves' candidates.
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(4))) struct SelDesc CSel;
typedef const __attribute__((address_space(4))) struct SelCol CSelCol;

__device__ __forceinline__ bool sel_less(uint64_t ak, uint64_t ar, uint64_t bk, uint64_t br) {
  return ak < bk || (ak == bk && ar < br);
}
__device__ __forceinline__ u64x2 sel_load(const SelEnt* e, uint64_t i) { return ((const AS1 u64x2*)e)[i]; }
__device__ __forceinline__ void sel_store(SelEnt* e, uint64_t i, uint64_t key, uint64_t row) {
  u64x2 v;
  v.x = key;
  v.y = row;
  ((AS1 u64x2*)e)[i] = v;
}

// The threads of one radix select meet: a wave on its own (NT == 64: its LDS operations and its loads and stores are
// ordered by the waits of the two fences; nothing else shares its state), or a workgroup of NT threads.
template <int NT>
__device__ __forceinline__ void sel_sync() {
  if constexpr (NT == kWave) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  } else {
    __syncthreads();
  }
}

// The entry of 0-based `rank` in ascending order among the entries `each` enumerates (all distinct: rows are), found
// byte by byte from the top: per byte, the entries that share the bytes found so far count their digit in st[0..256),
// and the digit at which the running count passes the rank is the entry's. Bytes no entry uses (key_bits, row_bits)
// are skipped. each(f) calls f(key, row) for this thread's share of the entries; st: kSelLdsWords LDS words.
template <int NT, class Each>
__device__ __forceinline__ void sel_threshold(Each each, uint32_t rank, int key_bits, int row_bits, lds_u32_t* st,
                                              int tid, uint64_t& tk, uint64_t& tr) {
  tk = 0;
  tr = 0;
  for (int p = 15; p >= 0; --p) {
    const bool iskey = p >= 8;
    const int sh = 8 * (p & 7);
    if (sh >= (iskey ? key_bits : row_bits)) continue;
    for (int b = tid; b < 256; b += NT) st[b] = 0u;
    sel_sync<NT>();
    const uint64_t ck = tk, cr = tr;
    each([&](uint64_t k, uint64_t r) {
      bool in;
      uint32_t d;
      if (iskey) {
        in = sh == 56 || (k >> (sh + 8)) == (ck >> (sh + 8));
        d = (uint32_t)(k >> sh) & 255u;
      } else {
        in = k == ck && (sh == 56 || (r >> (sh + 8)) == (cr >> (sh + 8)));
        d = (uint32_t)(r >> sh) & 255u;
      }
      if (in) __hip_atomic_fetch_add(st + d, 1u, WG_RLX);
    });
    sel_sync<NT>();
    if (tid < kWave) {  // (one wave: lane l holds digits 4l .. 4l + 3)
      const uint32_t c0 = st[4 * tid], c1 = st[4 * tid + 1], c2 = st[4 * tid + 2], c3 = st[4 * tid + 3];
      const uint32_t s = c0 + c1 + c2 + c3;
      uint32_t incl = s;
#pragma unroll
      for (int o = 1; o < kWave; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)incl, o, kWave);
        if (tid >= o) incl += t;
      }
      const uint32_t excl = incl - s;
      if (rank >= excl && rank < incl) {
        uint32_t r = rank - excl, d = 4u * (uint32_t)tid;
        if (r >= c0) {
          r -= c0;
          ++d;
          if (r >= c1) {
            r -= c1;
            ++d;
            if (r >= c2) {
              r -= c2;
              ++d;
            }
          }
        }
        st[256] = d;
        st[257] = r;
      }
    }
    sel_sync<NT>();
    const uint32_t d = st[256];
    rank = st[257];
    if (iskey) tk |= (uint64_t)d << sh;
    else tr |= (uint64_t)d << sh;
  }
}

// A wave's full candidate segment e[0..n) compacted in place to its K smallest entries (n > K), order kept; (tk, tr) =
// the largest of them. Chunks of 64: every lane's entry of a chunk is loaded before any is stored (one load
// instruction, waited for by the store's data), and a chunk's stores land at or below its own entries.
__device__ __noinline__ u64x2 sel_compact(SelEnt* e, uint32_t n, uint32_t K, int key_bits, int row_bits, uint32_t st_lds,
                                          int lane) {
  lds_u32_t* st = (lds_u32_t*)(uintptr_t)st_lds;
  uint64_t tk, tr;
  auto each = [&](auto f) {
    for (uint32_t i = (uint32_t)lane; i < n; i += kWave) {
      const u64x2 v = sel_load(e, i);
      f(v.x, v.y);
    }
  };
  sel_threshold<kWave>(each, K - 1u, key_bits, row_bits, st, lane, tk, tr);
  uint32_t w = 0;
  for (uint32_t base = 0; base < n; base += kWave) {
    const uint32_t i = base + (uint32_t)lane;
    u64x2 v;
    v.x = ~0ull;
    v.y = ~0ull;
    if (i < n) v = sel_load(e, i);
    const bool keep = i < n && !sel_less(tk, tr, v.x, v.y);  // entry <= threshold
    const uint64_t km = __ballot(keep);
    const uint32_t r = __builtin_amdgcn_mbcnt_hi((uint32_t)(km >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)km, 0u));
    if (keep) sel_store(e, w + r, v.x, v.y);
    w += (uint32_t)__builtin_popcountll(km);
  }
  sel_sync<kWave>();
  u64x2 t;
  t.x = tk;
  t.y = tr;
  return t;
}

// ORDER BY component j of one doc, in place in the key (DevQuery::sel: SelPart). Double.compare order for floating
// values: every NaN the canonical one, then sign-magnitude bits mapped to unsigned order.
__device__ __forceinline__ uint64_t sel_component(CSelCol* cp, int width, int shift, int desc, const uint32_t* img,
                                                  int doc_local, int64_t doc) {
  if (width == 0) return 0ull;  // a dictionary of one value
  CSelCol& c = *cp;
  uint64_t v;
  if (c.kind == COL_SV_DICT) {
    uint32_t id = c.lds_off >= 0 ? decode_lds(img + c.lds_off, doc_local, c.nbits) : decode_global(c.words, doc, c.nbits);
    if (c.remap != nullptr) id = (uint32_t)gp(c.remap)[id];
    v = id;
  } else {
    switch (c.vtype) {
      case PA_INT: v = (uint32_t)gp((const int32_t*)c.raw)[doc] ^ 0x80000000u; break;
      case PA_LONG: v = (uint64_t)gp((const int64_t*)c.raw)[doc] ^ 0x8000000000000000ull; break;
      case PA_FLOAT: {
        uint32_t b = gp((const uint32_t*)c.raw)[doc];
        if ((b & 0x7fffffffu) > 0x7f800000u) b = 0x7fc00000u;
        v = (b & 0x80000000u) ? (uint32_t)~b : (b | 0x80000000u);
      } break;
      default: {
        uint64_t b = gp((const uint64_t*)c.raw)[doc];
        if ((b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) b = 0x7ff8000000000000ull;
        v = (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
      } break;
    }
  }
  if (desc) v = ~v & (width >= 64 ? ~0ull : ((1ull << width) - 1ull));
  return v << shift;
}

// The docs of one tile that passed the filter (bit i of m: the lane's doc of step i) offered to the wave's candidates.
template <int STEPS, int LM>
__device__ __forceinline__ void select_tile(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                            const uint32_t* img, int64_t doc_base, uint32_t m, int lane, WaveState& la) {
  CSel* S = (CSel*)(uintptr_t)q->sel;
  const int nob = S->nob;
  const uint32_t K = (uint32_t)S->K, CAP = (uint32_t)S->cap;
  CSelCol* cols = (CSelCol*)(uintptr_t)(S->ob_cols + (size_t)seg->index * nob);
  SelEnt* e = S->scratch + (uint64_t)la.leap_slice * CAP;
  const uint64_t gb = __hip_atomic_load(gp(S->bound), RLX);
  const uint64_t seg_row = (uint64_t)(uint32_t)seg->index << 32;
  for (int i = 0; i < STEPS; ++i) {
    const bool act = ((m >> i) & 1u) != 0;
    if (__ballot(act) == 0) continue;
    const int dl = LM ? 32 * lane + i : i * kWave + lane;
    const int64_t doc = doc_base + dl;
    uint64_t key = 0;
    if (act)
      for (int j = 0; j < nob; ++j)
        key |= sel_component(cols + j, S->part[j].width, S->part[j].shift, S->part[j].desc, img, dl, doc);
    const uint64_t row = seg_row | (uint64_t)doc;
    // strictly below the wave's bound (an all-ones key is still below the initial all-ones bound: its row is not)
    bool pass = act && key <= gb && sel_less(key, row, la.sel_bk, la.sel_br);
    for (;;) {
      const uint64_t pm = __ballot(pass);
      if (pm == 0) break;
      const uint32_t r = __builtin_amdgcn_mbcnt_hi((uint32_t)(pm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)pm, 0u));
      const uint32_t room = CAP - la.sel_n;
      const bool take = pass && r < room;
      if (take) sel_store(e, la.sel_n + r, key, row);
      const uint32_t want = (uint32_t)__builtin_popcountll(pm);
      const uint32_t tk = want < room ? want : room;
      la.sel_n = (uint32_t)__builtin_amdgcn_readfirstlane((int)(la.sel_n + tk));
      la.sel_app += tk;
      pass = pass && !take;
      if (la.sel_n == CAP) {
        const u64x2 t = sel_compact(e, CAP, K, S->key_bits, S->row_bits, la.sel_lds, lane);
        la.sel_n = K;
        la.sel_bk = t.x;
        la.sel_br = t.y;
        ++la.sel_cmp;
        if (lane == 0) __hip_atomic_fetch_min(gp(S->bound), (unsigned long long)t.x, RLX);
        pass = pass && sel_less(key, row, t.x, t.y);
      }
    }
  }
}

// Start of the kernel: no candidate yet, the bound all ones; the wave's select state in LDS.
__device__ __forceinline__ void sel_state_init(WaveState& la, const uint32_t* smem, int wave) {
  la.sel_n = la.sel_app = la.sel_cmp = 0u;
  la.sel_bk = la.sel_br = ~0ull;
  la.sel_lds = lds_addr(smem) + (uint32_t)wave * (uint32_t)(kSelLdsWords * 4);
}

// End of a segment run: the segment's matched docs (its share of numEntriesScannedPostFilter).
__device__ __forceinline__ void sel_segment_docs(const DevQuery* q, const DevSeg* seg, uint32_t matched,
                                                 uint32_t matched_seg0, int lane) {
  const int64_t sm = wave_sum_i64((int64_t)(matched - matched_seg0));
  if (lane == 0 && sm != 0) __hip_atomic_fetch_add(gp(q->sel->seg_docs) + seg->index, (unsigned long long)sm, RLX);
}

// End of the kernel, every wave: the finish kernels read every wave's count.
__device__ __forceinline__ void sel_counters_flush(const DevQuery* q, const WaveState& la, int lane) {
  if (lane == 0) {
    gp(q->sel->wave_n)[la.leap_slice] = la.sel_n;
    if (la.sel_app) __hip_atomic_fetch_add(gp(q->sel->counters), (unsigned long long)la.sel_app, RLX);
    if (la.sel_cmp) __hip_atomic_fetch_add(gp(q->sel->counters) + 1, (unsigned long long)la.sel_cmp, RLX);
  }
}

}  // namespace pa
