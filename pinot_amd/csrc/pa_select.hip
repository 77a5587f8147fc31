// Selection queries (SELECT columns ... ORDER BY ... LIMIT), everything but the scan strategy itself
// (pa_strat_select.h "selection", pa_scan_select.hip): the C-ABI entry points, the planner's part, and the finish
// kernels that turn the scan waves' candidates into the result — gather the candidates the final bound admits, select
// the K smallest (the same radix select the waves compact with, one workgroup), sort them (bitonic, in global memory:
// K <= 65536), decode the output cells. Reference: SelectionOrderByOperator.java:193-322 (the queue drained into rows, the non-ordered
// columns fetched for the kept docs only) and SelectionOrderByCombineOperator (the segments' queues merged).
#include "pa_host.h"
#include "pa_strat_select.h"

namespace pa {

constexpr int kSelGatherThreads = 256;
constexpr int kSelFinishThreads = 1024;

// Every candidate whose key the final bound admits, from every wave's segment into one array (order does not matter:
// the result is selected and sorted from it).
__global__ void __launch_bounds__(kSelGatherThreads) select_gather_kernel(const SelDesc* __restrict__ S) {
  const uint64_t gb = *gp(S->bound);
  const uint32_t cap = (uint32_t)S->cap;
  for (int w = blockIdx.x; w < S->waves; w += gridDim.x) {
    const uint32_t n = gp(S->wave_n)[w];
    const SelEnt* src = S->scratch + (uint64_t)w * cap;
    for (uint32_t i = threadIdx.x; i < n && i < cap; i += kSelGatherThreads) {
      const u64x2 v = sel_load(src, i);
      if (v.x > gb) continue;
      const uint64_t pos = __hip_atomic_fetch_add(gp(S->cursor), 1ull, RLX);
      sel_store(S->cand, pos, v.x, v.y);
    }
  }
}

// One workgroup: the min(K, candidates) smallest candidates, ascending, into S->sorted.
__global__ void __launch_bounds__(kSelFinishThreads) select_finish_kernel(const SelDesc* __restrict__ S) {
  __shared__ uint32_t st_mem[kSelLdsWords];
  __shared__ uint32_t cur;
  const int tid = threadIdx.x;
  const uint64_t M = *gp(S->cursor);
  const uint64_t R = M < (uint64_t)S->K ? M : (uint64_t)S->K;
  if (R == 0) {
    if (tid == 0) *gp(S->result_n) = 0u;
    return;
  }
  const SelEnt* cand = S->cand;
  uint64_t tk = ~0ull, tr = ~0ull;  // (fewer candidates than K: every one of them is at or below all ones)
  if (M > R) {
    auto each = [&](auto f) {
      for (uint64_t i = (uint64_t)tid; i < M; i += kSelFinishThreads) {
        const u64x2 v = sel_load(cand, i);
        f(v.x, v.y);
      }
    };
    sel_threshold<kSelFinishThreads>(each, (uint32_t)(R - 1), S->key_bits, S->row_bits, lds_ptr(st_mem), tid, tk, tr);
  }
  if (tid == 0) cur = 0u;
  __syncthreads();
  SelEnt* out = S->sorted;
  for (uint64_t i = (uint64_t)tid; i < M; i += kSelFinishThreads) {
    const u64x2 v = sel_load(cand, i);
    if (sel_less(tk, tr, v.x, v.y)) continue;
    const uint32_t pos = atomicAdd(&cur, 1u);
    if (pos < R) sel_store(out, pos, v.x, v.y);
  }
  uint64_t N = 2;  // the sorted array: R entries padded with all ones to a power of two
  while (N < R) N <<= 1;
  for (uint64_t i = R + (uint64_t)tid; i < N; i += kSelFinishThreads) sel_store(out, i, ~0ull, ~0ull);
  __syncthreads();
  for (uint64_t k = 2; k <= N; k <<= 1)
    for (uint64_t j = k >> 1; j > 0; j >>= 1) {
      for (uint64_t i = (uint64_t)tid; i < N; i += kSelFinishThreads) {
        const uint64_t l = i ^ j;
        if (l <= i) continue;
        const u64x2 a = sel_load(out, i), b = sel_load(out, l);
        const bool up = (i & k) == 0;
        if (sel_less(b.x, b.y, a.x, a.y) == up) {
          sel_store(out, i, b.x, b.y);
          sel_store(out, l, a.x, a.y);
        }
      }
      __syncthreads();
    }
  if (tid == 0) *gp(S->result_n) = (uint32_t)R;
}

// One cell: the segment's dictId of a dictionary column (bit-unpacked at `doc`), the value of a raw column (FLOAT
// widened: the cell holds the bits of a double). Shared by the selection's cells and the row-by-time finish.
__device__ __forceinline__ int64_t sel_read_cell(const SelCol& col, int64_t doc) {
  if (col.kind == COL_SV_DICT) return (int64_t)decode_global(col.words, doc, col.nbits);
  switch (col.vtype) {
    case PA_INT: return (int64_t)gp((const int32_t*)col.raw)[doc];
    case PA_LONG: return gp((const int64_t*)col.raw)[doc];
    case PA_FLOAT: return __builtin_bit_cast(int64_t, (double)gp((const float*)col.raw)[doc]);
    default: return gp((const int64_t*)col.raw)[doc];
  }
}

// Output cell (row r, column c) at (segment, doc) of the sorted result.
__global__ void __launch_bounds__(kSelGatherThreads) select_cells_kernel(const SelDesc* __restrict__ S) {
  const uint64_t R = *gp(S->result_n);
  const uint64_t nout = (uint64_t)S->nout, K = (uint64_t)S->K;
  for (uint64_t idx = (uint64_t)blockIdx.x * kSelGatherThreads + threadIdx.x; idx < R * nout;
       idx += (uint64_t)gridDim.x * kSelGatherThreads) {
    const uint64_t c = idx / R, r = idx % R;
    const u64x2 v = sel_load(S->sorted, r);
    const uint64_t seg = v.y >> 32;
    const int64_t doc = (int64_t)(v.y & 0xffffffffull);
    const SelCol col = S->out_cols[seg * nout + c];
    gp(S->cells)[c * K + r] = sel_read_cell(col, doc);
  }
}

// FIRSTWITHTIME / LASTWITHTIME finish (pa_query_fetch_time_rows): one thread per (group, column) over the compacted
// group order of pa_query_fetch. words[keys[g]] & row_mask = row + 1 of group g's winning doc (0: no row), row = segment
// bind index << doc_bits | docId; the thread of column 0 also writes the row's (segment, doc). Cell c of group g goes
// to cells[c * n + g] (0 for a group with no row).
__global__ void __launch_bounds__(kSelGatherThreads)
    time_rows_kernel(const uint64_t* __restrict__ words, const int64_t* __restrict__ keys, int64_t n, int ncol,
                     uint64_t row_mask, int doc_bits, int nseg, const SelCol* __restrict__ cols, int32_t* __restrict__ out_seg,
                     int32_t* __restrict__ out_doc, int64_t* __restrict__ cells) {
  const int64_t per = ncol > 0 ? ncol : 1;
  for (int64_t idx = (int64_t)blockIdx.x * kSelGatherThreads + threadIdx.x; idx < n * per;
       idx += (int64_t)gridDim.x * kSelGatherThreads) {
    const int64_t c = idx / n, g = idx % n;
    const uint64_t r1 = gp(words)[gp(keys)[g]] & row_mask;
    int64_t seg = -1, doc = -1;
    if (r1 != 0) {
      seg = (int64_t)((r1 - 1) >> doc_bits);
      doc = (int64_t)((r1 - 1) & ((1ull << doc_bits) - 1ull));
    }
    if (seg >= nseg) seg = doc = -1;  // (cannot happen: the scan builds rows of bound segments only)
    if (c == 0) {
      gp(out_seg)[g] = (int32_t)seg;
      gp(out_doc)[g] = (int32_t)doc;
    }
    if (ncol > 0) gp(cells)[c * n + g] = seg >= 0 ? sel_read_cell(cols[seg * ncol + c], doc) : 0;
  }
}

}  // namespace pa

// ---------------------------------------------------------------- planning
static const Column* select_column(const pa_query* q, int si, int32_t cid) {
  auto it = q->segs[si]->cols.find(cid);
  return it == q->segs[si]->cols.end() ? nullptr : it->second;
}

static int select_check_column(const pa_query* q, int32_t cid, bool want_raw, bool ordered, const char* what) {
  for (int si = 0; si < q->nseg; ++si) {
    const Column* c = select_column(q, si, cid);
    const std::string name = std::string(what) + " column " + std::to_string(cid);
    if (!c) return fail(PA_EINVAL, "selection: " + name + " missing in segment " + std::to_string(si));
    if (c->kind == COL_MV_DICT) return fail(PA_EUNSUPPORTED, "selection: multi-value " + name + " is not supported");
    if (c->vtype == PA_BYTES) return fail(PA_EUNSUPPORTED, "selection: BYTES " + name + " is not supported");
    if (c->kind != COL_SV_DICT && c->kind != COL_SV_RAW) return fail(PA_EINVAL, "selection: bad " + name);
    if (ordered && (c->kind == COL_SV_RAW) != want_raw)
      return fail(PA_EUNSUPPORTED, "selection: " + name + " is dictionary-encoded in some segments only, or its "
                                   "order_by_cardinality does not say which it is");
    if (c->kind == COL_SV_RAW && (c->vtype < PA_INT || c->vtype > PA_DOUBLE))
      return fail(PA_EUNSUPPORTED, "selection: raw " + name + " of a type without an order");
  }
  return PA_OK;
}

// A column of one segment as the finish kernels read its cells (no remap, not staged).
static void select_describe(const Column* c, SelCol& o) {
  o.words = c->words.p ? (const uint32_t*)c->words.p + kGuardWords : nullptr;
  o.raw = c->raw.p;
  o.remap = nullptr;
  o.kind = c->kind;
  o.nbits = c->nbits;
  o.vtype = c->vtype;
  o.lds_off = -1;
}

int select_validate(pa_query* q) {
  const pa_select_spec& sp = q->sel_spec;
  SelDesc& d = q->hsel;
  std::memset(&d, 0, sizeof(d));
  if (q->nseg == 0) return fail(PA_EINVAL, "selection: no segment bound");
  int bits = 0;
  for (int j = 0; j < sp.num_order_by; ++j) {
    const bool raw = sp.order_by_cardinality[j] == 0;
    if (int rc = select_check_column(q, sp.order_by_columns[j], raw, true, "order-by")) return rc;
    const Column* c0 = select_column(q, 0, sp.order_by_columns[j]);
    int w;
    if (raw) {
      for (int si = 1; si < q->nseg; ++si)
        if (select_column(q, si, sp.order_by_columns[j])->vtype != c0->vtype)
          return fail(PA_EINVAL, "selection: order-by column " + std::to_string(sp.order_by_columns[j]) +
                                 " has different types in different segments");
      w = (c0->vtype == PA_INT || c0->vtype == PA_FLOAT) ? 32 : 64;
    } else {
      const uint64_t card = (uint64_t)sp.order_by_cardinality[j];
      for (int si = 0; si < q->nseg; ++si)
        if (q->sel_remaps[si][j].empty() &&
            (uint64_t)select_column(q, si, sp.order_by_columns[j])->cardinality > card)
          return fail(PA_EINVAL, "selection: a segment dictionary is larger than order_by_cardinality");
      w = card <= 1 ? 0 : 64 - __builtin_clzll(card - 1);
    }
    d.part[j].width = w;
    d.part[j].desc = sp.order_by_desc[j] ? 1 : 0;
    bits += w;
  }
  if (bits > 64)
    return fail(PA_EUNSUPPORTED, "selection: order-by key components wider than 64 bits together (" +
                                 std::to_string(bits) + ") are not supported");
  int shift = bits;  // most significant first
  for (int j = 0; j < sp.num_order_by; ++j) {
    shift -= d.part[j].width;
    d.part[j].shift = d.part[j].width ? shift : 0;
  }
  d.key_bits = bits;
  for (int c = 0; c < sp.num_columns; ++c)
    if (int rc = select_check_column(q, sp.columns[c], false, false, "select")) return rc;
  return PA_OK;
}

static int select_upload(pa_query* q, DevBuf& b, const void* host, size_t bytes) {
  dev_free(b);
  if (int rc = dev_alloc(b, bytes)) return rc;
  if (bytes) PA_HIP(hipMemcpy(b.p, host, bytes, hipMemcpyHostToDevice));
  return PA_OK;
}

int select_plan(pa_query* q) {
  const pa_select_spec& sp = q->sel_spec;
  SelDesc& d = q->hsel;
  const int64_t K = sp.num_rows;
  const int64_t cap_max = std::max<int64_t>(2 * K, 128);
  const int64_t cap = q->tune.select_cap > 0 ? q->tune.select_cap : cap_max;
  if (cap < K + 1 || cap > cap_max)
    return fail(PA_EINVAL, "tuning select_cap: " + std::to_string(cap) + " outside " + std::to_string(K + 1) + ".." +
                           std::to_string(cap_max));
  // the launch's waves: as many as the scratch bound lets own a candidate segment
  const int wpw = scan_waves(q->strategy);
  const int64_t max_waves = ((int64_t)q->tune.select_scratch_mib << 20) / (cap * (int64_t)sizeof(SelEnt));
  q->grid = (int)std::max<int64_t>(1, std::min<int64_t>(q->grid, max_waves / wpw));
  const int64_t waves = (int64_t)q->grid * wpw;
  d.nob = sp.num_order_by;
  d.nout = sp.num_columns;
  d.K = (int32_t)K;
  d.cap = (int32_t)cap;
  d.nseg = q->nseg;
  d.waves = (int32_t)waves;
  d.row_bits = 32 + (q->nseg > 1 ? 32 - __builtin_clz((uint32_t)(q->nseg - 1)) : 0);

  auto describe = [&](int si, int32_t cid, const std::vector<int32_t>* remap, SelCol& o) -> int {
    const Column* c = select_column(q, si, cid);
    select_describe(c, o);
    if (remap && !remap->empty()) {
      void* p = nullptr;
      if (int rc = upload_owned(q, remap->data(), remap->size() * sizeof(int32_t), &p)) return rc;
      o.remap = (const int32_t*)p;
    }
    if (remap && c->kind == COL_SV_DICT)  // an order-by column the filter stages is read from the tile image
      for (size_t sl = 0; sl < q->slot_cols.size(); ++sl)
        if (q->slot_cols[sl] == cid && q->hsegs[si].cols[sl].kind == COL_SV_DICT) o.lds_off = q->hsegs[si].cols[sl].lds_off;
    return PA_OK;
  };
  std::vector<SelCol> ob((size_t)q->nseg * std::max(1, d.nob)), out((size_t)q->nseg * std::max(1, d.nout));
  for (int si = 0; si < q->nseg; ++si) {
    for (int j = 0; j < d.nob; ++j)
      if (int rc = describe(si, sp.order_by_columns[j], &q->sel_remaps[si][j], ob[(size_t)si * d.nob + j])) return rc;
    for (int c = 0; c < d.nout; ++c)
      if (int rc = describe(si, sp.columns[c], nullptr, out[(size_t)si * d.nout + c])) return rc;
  }
  void* p = nullptr;
  if (int rc = upload_owned(q, ob.data(), ob.size() * sizeof(SelCol), &p)) return rc;
  d.ob_cols = (const SelCol*)p;
  if (int rc = upload_owned(q, out.data(), out.size() * sizeof(SelCol), &p)) return rc;
  d.out_cols = (const SelCol*)p;

  const size_t hdr_words = 5 + (size_t)q->nseg;
  if (int rc = dev_alloc(q->sel_hdr, hdr_words * 8 + (size_t)waves * 4)) return rc;
  if (int rc = dev_alloc(q->sel_scratch, (size_t)waves * cap * sizeof(SelEnt))) return rc;
  if (int rc = dev_alloc(q->sel_cand, (size_t)waves * cap * sizeof(SelEnt))) return rc;
  size_t sorted_n = 2;
  while ((int64_t)sorted_n < K) sorted_n <<= 1;
  if (int rc = dev_alloc(q->sel_sorted, sorted_n * sizeof(SelEnt))) return rc;
  if (int rc = dev_alloc(q->sel_cells, (size_t)std::max(1, d.nout) * K * 8)) return rc;
  unsigned long long* h = (unsigned long long*)q->sel_hdr.p;
  d.bound = h;
  d.cursor = h + 1;
  d.counters = h + 2;
  d.result_n = (uint32_t*)(h + 4);
  d.seg_docs = h + 5;
  d.wave_n = (uint32_t*)(h + hdr_words);
  d.scratch = (SelEnt*)q->sel_scratch.p;
  d.cand = (SelEnt*)q->sel_cand.p;
  d.sorted = (SelEnt*)q->sel_sorted.p;
  d.cells = (int64_t*)q->sel_cells.p;
  if (int rc = select_upload(q, q->sel_desc, &d, sizeof(d))) return rc;
  q->hq.sel = (const SelDesc*)q->sel_desc.p;
  q->sel_seg_docs.assign(q->nseg, 0);
  q->sel_counters[2] = waves;
  q->sel_counters[3] = cap;
  PLAN_LOG("selection: K=%lld cap=%lld waves=%lld key bits %d", (long long)K, (long long)cap, (long long)waves, d.key_bits);
  return PA_OK;
}

int select_reset(pa_query* q, hipStream_t st) {
  PA_HIP(hipMemsetAsync(q->sel_hdr.p, 0, q->sel_hdr.n, st));
  PA_HIP(launch_fill_i64((int64_t*)q->hsel.bound, 1, -1, st));  // no wave has published a bound
  return PA_OK;
}

// ---------------------------------------------------------------- C-ABI
extern "C" {

int pa_query_set_selection(pa_query* q, const pa_select_spec* spec) {
  if (!q || !spec) return fail(PA_EINVAL, "bad selection arguments");
  if (q->prepared) return fail(PA_EINVAL, "query already prepared");
  for (const pa_segment* s : q->segs)
    if (s) return fail(PA_EINVAL, "set the selection before binding segments");
  if (q->spec.num_group_by != 0) return fail(PA_EINVAL, "a selection is made from an aggregation-only spec");
  if (spec->num_order_by < 0 || spec->num_order_by > PA_MAX_ORDER_BY || spec->num_columns < 0 ||
      spec->num_columns > PA_MAX_SELECT_COLUMNS)
    return fail(PA_EINVAL, "selection spec counts out of range");
  if (spec->num_rows < 1) return fail(PA_EINVAL, "selection: num_rows must be at least 1");
  if (spec->num_rows > PA_MAX_SELECT_ROWS)
    return fail(PA_EUNSUPPORTED, "selection: num_rows " + std::to_string(spec->num_rows) + " exceeds PA_MAX_SELECT_ROWS (" +
                                 std::to_string(PA_MAX_SELECT_ROWS) + ")");
  for (int j = 0; j < spec->num_order_by; ++j)
    if (spec->order_by_cardinality[j] < 0 || spec->order_by_cardinality[j] > INT32_MAX)
      return fail(PA_EINVAL, "selection: bad order_by_cardinality");
  q->is_select = true;
  q->sel_spec = *spec;
  q->sel_remaps.assign(q->nseg, std::vector<std::vector<int32_t>>(spec->num_order_by));
  return PA_OK;
}

int pa_query_bind_order_remap(pa_query* q, int32_t segment_index, int32_t order_by_index, const int32_t* remap) {
  if (!q || !q->is_select || segment_index < 0 || segment_index >= q->nseg || order_by_index < 0 ||
      order_by_index >= q->sel_spec.num_order_by)
    return fail(PA_EINVAL, "bad order remap arguments");
  if (q->prepared) return fail(PA_EINVAL, "query already prepared");
  if (!q->segs[segment_index]) return fail(PA_EINVAL, "bind the segment before its order remaps");
  std::vector<int32_t>& rm = q->sel_remaps[segment_index][order_by_index];
  rm.clear();
  if (!remap) return PA_OK;
  const int64_t card = q->sel_spec.order_by_cardinality[order_by_index];
  if (card == 0) return fail(PA_EINVAL, "a raw order-by column takes no remap");
  auto it = q->segs[segment_index]->cols.find(q->sel_spec.order_by_columns[order_by_index]);
  if (it == q->segs[segment_index]->cols.end()) return fail(PA_EINVAL, "order-by column missing in segment");
  rm.assign(remap, remap + it->second->cardinality);
  for (int32_t v : rm)
    if (v < 0 || v >= card) {
      rm.clear();
      return fail(PA_EINVAL, "order remap id outside the table-wide dictionary");
    }
  return PA_OK;
}

int64_t pa_query_fetch_selection(pa_query* q, void* stream, int64_t capacity, int32_t* out_segments, int32_t* out_docs,
                                 uint64_t* out_keys, int64_t* const* out_cells) {
  if (!q || !q->prepared) return fail(PA_EINVAL, "query not prepared");
  if (!q->is_select) return fail(PA_EINVAL, "not a selection query");
  if (capacity < 0) return fail(PA_EINVAL, "negative capacity");
  hipStream_t st = (hipStream_t)stream;
  const SelDesc& d = q->hsel;
  const SelDesc* dd = (const SelDesc*)q->sel_desc.p;
  const size_t hdr_words = 5 + (size_t)q->nseg;
  std::vector<uint64_t> hdr(hdr_words, 0);
  uint64_t md[4] = {0, 0, 0, 0};
  if (q->num_tiles != 0) {
    PA_HIP(hipMemsetAsync(d.cursor, 0, 8, st));
    hipLaunchKernelGGL(select_gather_kernel, dim3((unsigned)std::min<int64_t>(d.waves, 2048)), dim3(kSelGatherThreads), 0,
                       st, dd);
    hipLaunchKernelGGL(select_finish_kernel, dim3(1), dim3(kSelFinishThreads), 0, st, dd);
    const int64_t cells = (int64_t)d.K * d.nout;
    if (cells > 0)
      hipLaunchKernelGGL(select_cells_kernel,
                         dim3((unsigned)std::min<int64_t>(1024, (cells + kSelGatherThreads - 1) / kSelGatherThreads)),
                         dim3(kSelGatherThreads), 0, st, dd);
    PA_HIP(hipGetLastError());
    PA_HIP(hipMemcpyAsync(hdr.data(), q->sel_hdr.p, hdr_words * 8, hipMemcpyDeviceToHost, st));
  }
  PA_HIP(hipMemcpyAsync(md, q->sections.back().ptr, 32, hipMemcpyDeviceToHost, st));
  PA_HIP(hipStreamSynchronize(st));
  q->last_matched = (int64_t)md[0];
  q->scanned_since_fetch = false;
  q->sel_counters[0] = (int64_t)hdr[2];
  q->sel_counters[1] = (int64_t)hdr[3];
  for (int si = 0; si < q->nseg; ++si) q->sel_seg_docs[si] = (int64_t)hdr[5 + si];
  const int64_t R = (int64_t)(uint32_t)hdr[4];
  const int64_t n = std::min(R, capacity);
  if (n > 0) {
    std::vector<SelEnt> rows((size_t)n);
    PA_HIP(hipMemcpyAsync(rows.data(), q->sel_sorted.p, (size_t)n * sizeof(SelEnt), hipMemcpyDeviceToHost, st));
    for (int c = 0; c < d.nout; ++c)
      if (out_cells && out_cells[c])
        PA_HIP(hipMemcpyAsync(out_cells[c], (const int64_t*)q->sel_cells.p + (size_t)c * d.K, (size_t)n * 8,
                              hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    for (int64_t r = 0; r < n; ++r) {
      if (out_segments) out_segments[r] = (int32_t)(rows[r].row >> 32);
      if (out_docs) out_docs[r] = (int32_t)(uint32_t)rows[r].row;
      if (out_keys) out_keys[r] = rows[r].key;
    }
  }
  return R;
}

int pa_query_fetch_time_rows(pa_query* q, void* stream, int32_t agg, int64_t num_groups, int32_t num_columns,
                             const int32_t* columns, int32_t* out_segments, int32_t* out_docs, int64_t* const* out_cells) {
  if (!q || !q->prepared) return fail(PA_EINVAL, "query not prepared");
  if (const char* t = tuning_invalidating(q->tune))
    return fail(PA_EINVAL, std::string("results invalid: tuning ") + t + " is set");
  if (agg < 0 || agg >= q->spec.num_aggs || !q->trow_form[agg])
    return fail(PA_EINVAL, "not a LAST / FIRST_ROW_BY_TIME aggregation");
  if (q->hashed || q->agg_section[agg] < 0) return fail(PA_EINVAL, "internal: time rows without a direct key space");
  if (num_groups < 0 || num_groups > INT32_MAX || num_columns < 0 || num_columns > PA_MAX_SELECT_COLUMNS ||
      (num_columns > 0 && !columns))
    return fail(PA_EINVAL, "fetch time rows: bad sizes");
  for (int c = 0; c < num_columns; ++c)
    if (int rc = select_check_column(q, columns[c], false, false, "row-by-time")) return rc;
  hipStream_t st = (hipStream_t)stream;
  // the keys pa_query_fetch returns for these accumulators: the same compaction passes
  const int64_t K = q->num_keys;
  const int64_t nb = (K + 2047) / 2048;
  if ((int64_t)q->fetch_blocks.n < (nb + 1) * 4) {
    dev_free(q->fetch_blocks);
    if (int rc = dev_alloc(q->fetch_blocks, (size_t)(nb + 1) * 4)) return rc;
  }
  const int all = q->spec.num_group_by != 0 ? 0 : 1;
  const unsigned long long* count = (const unsigned long long*)q->sections[0].ptr;
  uint32_t total = 0;
  PA_HIP(launch_compact(count, K, all, (uint32_t*)q->fetch_blocks.p, 0, nullptr, 0, st));
  PA_HIP(hipMemcpyAsync(&total, (uint32_t*)q->fetch_blocks.p + nb, 4, hipMemcpyDeviceToHost, st));
  PA_HIP(hipStreamSynchronize(st));
  if ((int64_t)total != num_groups)
    return fail(PA_EINVAL, "num_groups is not the group count pa_query_fetch returns for these accumulators");
  if (num_groups == 0) return PA_OK;
  // keys | segments | docs | cells [column][group] | column descriptors [segment][column]
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t n = (size_t)num_groups, nc = (size_t)num_columns;
  const size_t o_seg = al(n * 8), o_doc = o_seg + al(n * 4), o_cells = o_doc + al(n * 4);
  const size_t o_cols = o_cells + al(n * nc * 8);
  const size_t bytes = o_cols + al((size_t)q->nseg * nc * sizeof(SelCol));
  if (q->trow_buf.n < bytes || !q->trow_buf.p) {
    dev_free(q->trow_buf);
    if (int rc = dev_alloc(q->trow_buf, bytes)) return rc;
  }
  char* b = (char*)q->trow_buf.p;
  std::vector<SelCol> cols((size_t)q->nseg * nc);
  for (int si = 0; si < q->nseg; ++si)
    for (size_t c = 0; c < nc; ++c) select_describe(select_column(q, si, columns[c]), cols[(size_t)si * nc + c]);
  if (!cols.empty()) PA_HIP(hipMemcpy(b + o_cols, cols.data(), cols.size() * sizeof(SelCol), hipMemcpyHostToDevice));
  CompactDesc d;
  std::memset(&d, 0, sizeof(d));
  d.keys = (int64_t*)b;
  PA_HIP(launch_compact(count, K, all, (uint32_t*)q->fetch_blocks.p, num_groups, &d, 1, st));
  const int row_bits = q->trow_row_bits[agg];
  const uint64_t row_mask = (uint64_t(1) << row_bits) - 1;
  const int64_t threads = num_groups * std::max<int64_t>(1, num_columns);
  hipLaunchKernelGGL(time_rows_kernel,
                     dim3((unsigned)std::min<int64_t>(1024, (threads + kSelGatherThreads - 1) / kSelGatherThreads)),
                     dim3(kSelGatherThreads), 0, st, (const uint64_t*)q->sections[q->agg_section[agg]].ptr,
                     (const int64_t*)b, num_groups, (int)num_columns, row_mask, q->trow_doc_bits[agg], q->nseg,
                     (const SelCol*)(b + o_cols), (int32_t*)(b + o_seg), (int32_t*)(b + o_doc), (int64_t*)(b + o_cells));
  PA_HIP(hipGetLastError());
  if (out_segments) PA_HIP(hipMemcpyAsync(out_segments, b + o_seg, n * 4, hipMemcpyDeviceToHost, st));
  if (out_docs) PA_HIP(hipMemcpyAsync(out_docs, b + o_doc, n * 4, hipMemcpyDeviceToHost, st));
  for (size_t c = 0; c < nc; ++c)
    if (out_cells && out_cells[c])
      PA_HIP(hipMemcpyAsync(out_cells[c], b + o_cells + c * n * 8, n * 8, hipMemcpyDeviceToHost, st));
  PA_HIP(hipStreamSynchronize(st));
  return PA_OK;
}

int pa_query_selection_segment_docs(const pa_query* q, int64_t* out) {
  if (!q || !q->prepared || !q->is_select || !out) return fail(PA_EINVAL, "not a prepared selection query");
  for (int si = 0; si < q->nseg; ++si) out[si] = q->sel_seg_docs[si];
  return PA_OK;
}

int pa_query_selection_counters(const pa_query* q, int64_t* out) {
  if (!q || !q->prepared || !q->is_select || !out) return fail(PA_EINVAL, "not a prepared selection query");
  for (int i = 0; i < 4; ++i) out[i] = q->sel_counters[i];
  return PA_OK;
}

}  // extern "C"
