// Results: pa_query_fetch (compaction of the non-empty keys, one DMA per column), pa_query_fetch_trimmed (the same for
// the groups the server trim keeps, selected on the GPU: pa_trim.hip) and the hashed key space's row pack / merge for
// the cross-GPU exchange.
#include "pa_host.h"

// A query whose tunings skip work in a kernel (pa_query_results_invalid) can be executed and timed, not read
static int refuse_invalid(const pa_query* q) {
  const char* t = tuning_invalidating(q->tune);
  return t ? fail(PA_EINVAL, std::string("results invalid: tuning ") + t + " is set") : PA_OK;
}

// Filtered aggregations: out[j * n + g] = lane j's docs in fetched group g (PA_ACC_LANE_COUNT_U64 at keys[g]).
__global__ void __launch_bounds__(256) lane_count_gather_kernel(const unsigned long long* __restrict__ lane_count,
                                                                 int64_t num_keys, const int64_t* __restrict__ keys,
                                                                 int64_t n, int lanes, int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * lanes) return;
  const int64_t j = i / n, g = i - j * n;
  out[i] = (int64_t)lane_count[j * num_keys + keys[g]];
}

extern "C" {
int pa_query_fetch_lane_counts(pa_query* q, void* stream, int64_t num_groups, int64_t* out) {
  if (!q || !q->prepared) return fail(PA_EINVAL, "query not prepared");
  if (!q->is_filtered) return fail(PA_EINVAL, "not a query with aggregation filters");
  if (int rc = refuse_invalid(q)) return rc;
  if (num_groups < 0 || num_groups > INT32_MAX || (num_groups > 0 && !out)) return fail(PA_EINVAL, "fetch lane counts: bad sizes");
  hipStream_t st = (hipStream_t)stream;
  // the keys pa_query_fetch returns for the current accumulators: the same compaction passes as the fetch
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
  const int lanes = q->filt_spec.num_filters;
  const size_t out_at = ((size_t)num_groups * 8 + 255) & ~(size_t)255;
  const size_t bytes = out_at + (size_t)num_groups * lanes * 8;
  if (q->lane_buf.n < bytes || !q->lane_buf.p) {
    dev_free(q->lane_buf);
    if (int rc = dev_alloc(q->lane_buf, bytes)) return rc;
  }
  CompactDesc d;
  std::memset(&d, 0, sizeof(d));
  d.keys = (int64_t*)q->lane_buf.p;
  PA_HIP(launch_compact(count, K, all, (uint32_t*)q->fetch_blocks.p, num_groups, &d, 1, st));
  int64_t* dout = (int64_t*)((char*)q->lane_buf.p + out_at);
  const int64_t cells = num_groups * lanes;
  lane_count_gather_kernel<<<(unsigned)((cells + 255) / 256), 256, 0, st>>>(
      (const unsigned long long*)q->sections[q->lane_section].ptr, K, d.keys, num_groups, lanes, dout);
  PA_HIP(hipGetLastError());
  PA_HIP(hipMemcpyAsync(out, dout, (size_t)cells * 8, hipMemcpyDeviceToHost, st));
  PA_HIP(hipStreamSynchronize(st));
  return PA_OK;
}

int64_t pa_query_fetch(pa_query* q, void* stream, int64_t capacity, int64_t* out_keys, int64_t* out_counts,
                       void* const* out_aggs) {
  if (!q || !q->prepared) return fail(PA_EINVAL, "query not prepared");
  if (q->is_select) return fail(PA_EINVAL, "a selection query has no groups: read it with pa_query_fetch_selection");
  if (q->is_distinct) return fail(PA_EINVAL, "a distinct query has no groups: read it with pa_query_fetch_distinct");
  if (int rc = refuse_invalid(q)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const pa_query_spec& s = q->spec;
  const int64_t K = q->num_keys;
  const bool grouped = s.num_group_by != 0;
  char* dbase = (char*)(q->external_acc ? q->external_acc : q->acc.p);

  // Decodes `nrows` host rows into the caller's arrays: row r has key key_of(r, w) (word w < kw: two-word hashed keys
  // fill out_keys[2 n], out_keys[2 n + 1]), count hc[r] and the aggregation section rows at sec(section)[r * per]. Rows
  // with a zero count are skipped when `skip_empty`. `order` (optional) lists the rows to emit, in output order (hashed
  // key spaces: sorted by packed key).
  const int kw = q->hashed ? q->key_words : 1;
  auto decode = [&](int64_t nrows, const uint64_t* hc, const std::function<const char*(int)>& sec,
                    const std::function<int64_t(int64_t, int)>& key_of, bool skip_empty,
                    const std::vector<int64_t>* order) -> int64_t {
    const char* asec[PA_MAX_AGGS];  // section base per aggregation, resolved once (not per row)
    for (int a = 0; a < s.num_aggs; ++a) asec[a] = q->agg_section[a] >= 0 ? sec(q->agg_section[a]) : nullptr;
    int64_t n = 0;
    const int64_t total = order ? (int64_t)order->size() : nrows;
    for (int64_t oi = 0; oi < total; ++oi) {
      const int64_t r = order ? (*order)[oi] : oi;
      if (skip_empty && hc[r] == 0) continue;
      if (n < capacity) {
        if (out_keys)
          for (int w = 0; w < kw; ++w) out_keys[kw * n + w] = key_of(r, w);
        if (out_counts) out_counts[n] = (int64_t)hc[r];
        for (int a = 0; a < s.num_aggs; ++a) {
          if (!out_aggs || !out_aggs[a]) continue;
          const pa_agg_spec& A = s.aggs[a];
          if (A.type == PA_AGG_VALUE_HISTOGRAM) continue;  // 0 bytes per row: pa_query_fetch_histogram reads the bins
          if (time_row_agg(A.type)) continue;              // 0 bytes per row: pa_query_fetch_time_rows reads the rows
          if (moments_agg(A.type)) continue;               // 0 bytes per row: pa_query_fetch_moments reads the tuples
          double* outd = (double*)out_aggs[a];
          if (A.type == PA_AGG_COUNT) {
            outd[n] = (double)hc[r];
            continue;
          }
          const char* sp = asec[a];
          const int src = q->hq.aggs[a].src;
          if (A.type == PA_AGG_DISTINCTCOUNTHLL || A.type == PA_AGG_DISTINCTCOUNT) {
            const int64_t per = A.type == PA_AGG_DISTINCTCOUNT ? presence_stride(A) : int64_t(1) << A.log2m;
            uint8_t* o = (uint8_t*)out_aggs[a] + n * per;
            std::memcpy(o, (const uint8_t*)sp + r * per, (size_t)per);
          } else if (A.type == PA_AGG_SUM || A.type == PA_AGG_COUNT_MV) {
            const int64_t* hv = (const int64_t*)sp;
            // SRC_LONG: exact 96-bit total, rounded once (the reference's double of the exact sum)
            if (src == SRC_LONG) outd[n] = (double)(((__int128)hv[2 * r + 1] << 32) + (__int128)(uint64_t)hv[2 * r]);
            else outd[n] = src == SRC_INT ? (double)hv[r] : ((const double*)sp)[r];
          } else {  // MIN / MAX; empty aggregation-only result -> +/-inf (Min/MaxAggregationFunction DEFAULT_VALUE)
            const int64_t e8 = ((const int64_t*)sp)[r];
            if (hc[r] == 0) outd[n] = A.type == PA_AGG_MIN ? __builtin_inf() : -__builtin_inf();
            else outd[n] = src != SRC_DOUBLE ? (double)e8 : f64_order_decode(e8);
          }
        }
      }
      ++n;
    }
    return n;
  };

  // Small accumulator blocks (the common case: a few thousand keys): ONE device-to-host copy of the whole block into
  // pinned memory and one synchronisation, then compaction + decode on the host.
  if (q->acc.n <= kFetchWholeBlockBytes) {
    if (!q->host_acc) {
      if (hipHostMalloc(&q->host_acc, std::max<size_t>(q->acc.n, 16), hipHostMallocDefault) != hipSuccess) {
        q->host_acc = nullptr;
        return fail(PA_ENOMEM, "hipHostMalloc for the accumulator copy failed");
      }
    }
    PA_HIP(hipMemcpyAsync(q->host_acc, dbase, q->acc.n, hipMemcpyDeviceToHost, st));
    if (q->is_filtered && !q->filt_seg_docs_host.empty())  // (the lanes' per-segment docs ride on this synchronisation: pa_query_lane_docs)
      PA_HIP(hipMemcpyAsync(q->filt_seg_docs_host.data(), q->filt_seg_docs.p, q->filt_seg_docs_host.size() * 8,
                            hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    const char* hb = (const char*)q->host_acc;
    auto hsec = [&](int sec) { return hb + ((char*)q->sections[sec].ptr - dbase); };
    const uint64_t* docs = (const uint64_t*)hsec((int)q->sections.size() - 1);
    q->last_matched = (int64_t)docs[0];
    q->last_reached = (int64_t)docs[2];
    q->scanned_since_fetch = false;
    if (docs[1]) return fail(PA_EUNSUPPORTED, "group-key table overflow (more distinct groups than slots)");
    if (docs[3]) return fail(PA_EHIP, "internal: partitioned passes disagree on record counts");
    const uint64_t* hc = (const uint64_t*)hsec(0);
    if (q->hashed) {
      const int64_t* hk = (const int64_t*)hsec(q->keys_section);
      const int ks = kw == 2 ? 3 : 1;  // key-section words per slot
      std::vector<int64_t> order;
      for (int64_t r = 0; r < K; ++r)
        if (hc[r]) order.push_back(r);
      std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
        return hk[ks * a] != hk[ks * b] ? hk[ks * a] < hk[ks * b] : (kw == 2 && hk[ks * a + 1] < hk[ks * b + 1]);
      });
      return decode(K, hc, hsec, [&](int64_t r, int w) { return hk[ks * r + w]; }, false, &order);
    }
    return decode(K, hc, hsec, [](int64_t r, int) { return r; }, grouped, nullptr);
  }

  // Large key spaces: ordered compaction of the non-empty keys on the GPU (count + scan, then key ids and every
  // section's rows gathered into a staging block), one copy of the compacted rows, decode on the host.
  const int64_t nb = (K + 2047) / 2048;
  if ((int64_t)q->fetch_blocks.n < (nb + 1) * 4) {
    dev_free(q->fetch_blocks);
    int rc = dev_alloc(q->fetch_blocks, (size_t)(nb + 1) * 4);
    if (rc) return rc;
  }
  const int all = grouped ? 0 : 1;
  uint32_t total = 0;
  uint64_t md[4] = {0, 0, 0, 0};
  PA_HIP(launch_compact((const unsigned long long*)q->sections[0].ptr, K, all, (uint32_t*)q->fetch_blocks.p, 0,
                        nullptr, 0, st));
  PA_HIP(hipMemcpyAsync(&total, (uint32_t*)q->fetch_blocks.p + nb, 4, hipMemcpyDeviceToHost, st));
  PA_HIP(hipMemcpyAsync(md, q->sections.back().ptr, 32, hipMemcpyDeviceToHost, st));
  if (q->is_filtered && !q->filt_seg_docs_host.empty())
    PA_HIP(hipMemcpyAsync(q->filt_seg_docs_host.data(), q->filt_seg_docs.p, q->filt_seg_docs_host.size() * 8,
                          hipMemcpyDeviceToHost, st));
  PA_HIP(hipStreamSynchronize(st));
  q->last_matched = (int64_t)md[0];
  q->last_reached = (int64_t)md[2];
  q->scanned_since_fetch = false;
  if (md[1]) return fail(PA_EUNSUPPORTED, "group-key table overflow (more distinct groups than slots)");
  if (md[3]) return fail(PA_EHIP, "internal: partitioned passes disagree on record counts");
  const int64_t m = (int64_t)total;
  const int64_t rows_cap = std::min<int64_t>(m, std::max<int64_t>(capacity, 0));
  if (rows_cap == 0) return m;
  if (!q->hashed) {
    // Direct key space: the compaction writes the caller's representation (key ids, counts, doubles / register bytes)
    // into staging columns on the GPU, and each column goes to the caller's array in one copy (a DMA straight into
    // pinned memory when the caller's arrays are pinned: engine.py keeps a reused pinned output pool). No host decode.
    FinalDesc f;
    std::memset(&f, 0, sizeof(f));
    f.nagg = s.num_aggs;
    std::vector<size_t> off(s.num_aggs, 0);
    size_t bytes = ((size_t)rows_cap * 16 + 255) & ~(size_t)255;  // keys | counts
    for (int a = 0; a < s.num_aggs; ++a) {
      const pa_agg_spec& A = s.aggs[a];
      // (a PA_AGG_MOMENTS aggregation goes to the kernel as the other type with 0 bytes per row: it skips both alike)
      f.type[a] = moments_agg(A.type) ? PA_AGG_VALUE_HISTOGRAM : A.type;
      f.src[a] = q->hq.aggs[a].src;
      f.sec[a] = q->agg_section[a] >= 0 ? q->sections[q->agg_section[a]].ptr : nullptr;
      f.per[a] = A.type == PA_AGG_DISTINCTCOUNT ? presence_stride(A)
                 : (A.type == PA_AGG_VALUE_HISTOGRAM || time_row_agg(A.type) || moments_agg(A.type)) ? 0  // (nothing staged or copied)
                 : (A.type == PA_AGG_DISTINCTCOUNTHLL ? (int64_t(1) << A.log2m) : 8);
      off[a] = bytes;
      bytes += ((size_t)rows_cap * (size_t)f.per[a] + 255) & ~(size_t)255;
    }
    if (q->fetch_stage.n < bytes) {
      dev_free(q->fetch_stage);
      int rc = dev_alloc(q->fetch_stage, bytes);
      if (rc) return rc;
    }
    char* ds = (char*)q->fetch_stage.p;
    f.keys = (int64_t*)ds;
    f.counts = (int64_t*)(ds + (size_t)rows_cap * 8);
    for (int a = 0; a < s.num_aggs; ++a) f.out[a] = ds + off[a];
    PA_HIP(launch_compact_final((const unsigned long long*)q->sections[0].ptr, K, all,
                                (const uint32_t*)q->fetch_blocks.p, rows_cap, &f, st));
    if (out_keys) PA_HIP(hipMemcpyAsync(out_keys, f.keys, (size_t)rows_cap * 8, hipMemcpyDeviceToHost, st));
    if (out_counts) PA_HIP(hipMemcpyAsync(out_counts, f.counts, (size_t)rows_cap * 8, hipMemcpyDeviceToHost, st));
    for (int a = 0; a < s.num_aggs; ++a)
      if (out_aggs && out_aggs[a] && f.per[a] > 0)
        PA_HIP(hipMemcpyAsync(out_aggs[a], f.out[a], (size_t)rows_cap * (size_t)f.per[a], hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    return m;
  }
  // staging: keys | count | one block per aggregation section (rows x per x es), 256-byte aligned pieces
  CompactDesc d;
  std::memset(&d, 0, sizeof(d));
  std::vector<int> secs = {0};
  for (int a = 0; a < s.num_aggs; ++a)
    if (q->agg_section[a] >= 0 && s.aggs[a].type != PA_AGG_VALUE_HISTOGRAM) secs.push_back(q->agg_section[a]);
  if (q->hashed) secs.push_back(q->keys_section);
  // hashed key spaces: every non-empty slot is needed to sort by packed key before the capacity cut
  const int64_t rows_needed = q->hashed ? m : std::min<int64_t>(m, std::max<int64_t>(capacity, 0));
  std::vector<size_t> offs;
  const int64_t rows = rows_needed;
  size_t bytes = ((size_t)rows * 8 + 255) & ~(size_t)255;
  for (int sec : secs) {
    const Section& sc = q->sections[sec];
    const int es = (int)section_es(sc.kind);  // HLL registers / presence: one byte each
    const int64_t per = sc.n / K;
    offs.push_back(bytes);
    bytes += ((size_t)rows * per * es + 255) & ~(size_t)255;
  }
  if (q->fetch_stage.n < bytes) {
    dev_free(q->fetch_stage);
    int rc = dev_alloc(q->fetch_stage, bytes);
    if (rc) return rc;
    if (q->fetch_host) (void)hipHostFree(q->fetch_host);
    if (hipHostMalloc(&q->fetch_host, bytes, hipHostMallocDefault) != hipSuccess) {
      q->fetch_host = nullptr;
      return fail(PA_ENOMEM, "hipHostMalloc for the fetch staging failed");
    }
  }
  char* dstage = (char*)q->fetch_stage.p;
  d.nsec = (int32_t)secs.size();
  d.keys = (int64_t*)dstage;
  for (size_t i = 0; i < secs.size(); ++i) {
    const Section& sc = q->sections[secs[i]];
    d.es[i] = (int32_t)section_es(sc.kind);
    d.per[i] = sc.n / K;
    d.src[i] = sc.ptr;
    d.dst[i] = dstage + offs[i];
  }
  PA_HIP(launch_compact((const unsigned long long*)q->sections[0].ptr, K, all, (uint32_t*)q->fetch_blocks.p, rows,
                        &d, 1, st));
  PA_HIP(hipMemcpyAsync(q->fetch_host, dstage, bytes, hipMemcpyDeviceToHost, st));
  PA_HIP(hipStreamSynchronize(st));
  const char* hb = (const char*)q->fetch_host;
  const int64_t* hkeys = (const int64_t*)hb;
  std::map<int, const char*> hsec;
  for (size_t i = 0; i < secs.size(); ++i) hsec[secs[i]] = hb + offs[i];
  if (q->hashed) {  // rows are slots: emit them in packed-key order
    const int64_t* pk = (const int64_t*)hsec[q->keys_section];
    const int ks = kw == 2 ? 3 : 1;
    std::vector<int64_t> order(rows);
    for (int64_t r = 0; r < rows; ++r) order[r] = r;
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
      return pk[ks * a] != pk[ks * b] ? pk[ks * a] < pk[ks * b] : (kw == 2 && pk[ks * a + 1] < pk[ks * b + 1]);
    });
    order.resize(rows_cap);
    decode(rows, (const uint64_t*)hsec[0], [&](int sec) { return hsec[sec]; },
           [&](int64_t r, int w) { return pk[ks * r + w]; }, false, &order);
    return m;
  }
  decode(rows, (const uint64_t*)hsec[0], [&](int sec) { return hsec[sec]; }, [&](int64_t r, int) { return hkeys[r]; },
         false, nullptr);
  return m;
}

// Bytes of word `x < bound`'s digits that can differ between candidates (the passes above them are skipped)
static int bytes_below(uint64_t bound) {
  int b = 1;
  while (b < 8 && (bound - 1) >> (8 * b)) ++b;
  return b;
}

int64_t pa_query_fetch_trimmed(pa_query* q, void* stream, const pa_trim_spec* spec, int64_t capacity,
                               int64_t* out_keys, int64_t* out_counts, void* const* out_aggs,
                               int64_t* out_total_groups) {
  if (!q || !q->prepared) return fail(PA_EINVAL, "query not prepared");
  if (!spec) return fail(PA_EINVAL, "fetch trimmed: null spec");
  if (q->is_select || q->is_distinct) return fail(PA_EINVAL, "fetch trimmed: not a group-by query");
  if (int rc = refuse_invalid(q)) return rc;
  const pa_query_spec& s = q->spec;
  if (q->hashed) return fail(PA_EUNSUPPORTED, "device group trim needs a direct key space");
  if (q->is_filtered) return fail(PA_EUNSUPPORTED, "device group trim: the query has aggregation filters");
  for (int a = 0; a < s.num_aggs; ++a)
    if (s.aggs[a].type == PA_AGG_VALUE_HISTOGRAM)
      return fail(PA_EUNSUPPORTED, "device group trim: the query has a VALUE_HISTOGRAM aggregation");
  for (int a = 0; a < s.num_aggs; ++a)
    if (time_row_agg(s.aggs[a].type))
      return fail(PA_EUNSUPPORTED, "device group trim: the query has a LAST / FIRST_ROW_BY_TIME aggregation");
  for (int a = 0; a < s.num_aggs; ++a)
    if (moments_agg(s.aggs[a].type))
      return fail(PA_EUNSUPPORTED, "device group trim: the query has a PA_AGG_MOMENTS aggregation");
  if (spec->num_terms < 0) return fail(PA_EINVAL, "fetch trimmed: negative term count");
  if (spec->num_terms > PA_MAX_TRIM_TERMS) return fail(PA_EUNSUPPORTED, "device group trim: too many ORDER BY terms");
  const int64_t K = q->num_keys;
  TrimWordsDesc w;
  std::memset(&w, 0, sizeof(w));
  w.nterms = spec->num_terms;
  w.ngb = s.num_group_by;
  for (int j = 0; j < s.num_group_by; ++j) w.card[j] = s.group_by_cardinality[j];
  auto agg_is = [&](int a, int type) { return a >= 0 && a < s.num_aggs && s.aggs[a].type == type; };
  for (int e = 0; e < spec->num_terms; ++e) {
    const int a = spec->index[e], b = spec->index2[e];
    w.kind[e] = spec->kind[e];
    w.a[e] = a;
    w.b[e] = b;
    w.desc[e] = spec->desc[e] ? 1 : 0;
    switch (spec->kind[e]) {
      case PA_TRIM_KEY_COLUMN: {
        if (a < 0 || a >= s.num_group_by) return fail(PA_EINVAL, "fetch trimmed: bad group-by position");
        int64_t st = 1;
        for (int j = 0; j < a; ++j) st *= s.group_by_cardinality[j];
        w.kstride[e] = st;
        w.kcard[e] = s.group_by_cardinality[a];
        break;
      }
      case PA_TRIM_COUNT: break;
      case PA_TRIM_AGG:
        if (a < 0 || a >= s.num_aggs) return fail(PA_EINVAL, "fetch trimmed: bad aggregation index");
        if (!agg_is(a, PA_AGG_SUM) && !agg_is(a, PA_AGG_MIN) && !agg_is(a, PA_AGG_MAX))
          return fail(PA_EUNSUPPORTED, "device group trim orders by SUM / MIN / MAX aggregations only");
        break;
      case PA_TRIM_AVG:
        if (!agg_is(a, PA_AGG_SUM)) return fail(PA_EINVAL, "fetch trimmed: AVG needs a SUM aggregation");
        break;
      case PA_TRIM_RANGE:
        if (!agg_is(a, PA_AGG_MAX) || !agg_is(b, PA_AGG_MIN))
          return fail(PA_EINVAL, "fetch trimmed: RANGE needs a MAX and a MIN aggregation");
        break;
      default: return fail(PA_EINVAL, "fetch trimmed: unknown term kind");
    }
  }
  hipStream_t st = (hipStream_t)stream;
  const bool grouped = s.num_group_by != 0;
  const int all = grouped ? 0 : 1;
  const unsigned long long* count = (const unsigned long long*)q->sections[0].ptr;

  // candidates: how many non-empty groups there are (the fetch's own count + scan pass)
  const int64_t nb = (K + 2047) / 2048;
  if ((int64_t)q->fetch_blocks.n < (nb + 1) * 4) {
    dev_free(q->fetch_blocks);
    if (int rc = dev_alloc(q->fetch_blocks, (size_t)(nb + 1) * 4)) return rc;
  }
  uint32_t* blocks = (uint32_t*)q->fetch_blocks.p;
  uint32_t total = 0;
  uint64_t md[4] = {0, 0, 0, 0};
  PA_HIP(launch_compact(count, K, all, blocks, 0, nullptr, 0, st));
  PA_HIP(hipMemcpyAsync(&total, blocks + nb, 4, hipMemcpyDeviceToHost, st));
  PA_HIP(hipMemcpyAsync(md, q->sections.back().ptr, 32, hipMemcpyDeviceToHost, st));
  PA_HIP(hipStreamSynchronize(st));
  const int64_t n = (int64_t)total;
  if (out_total_groups) *out_total_groups = n;
  const int64_t trim = std::max<int64_t>(spec->trim, 0);
  if (n <= trim || !grouped) return pa_query_fetch(q, stream, capacity, out_keys, out_counts, out_aggs);
  q->last_matched = (int64_t)md[0];
  q->last_reached = (int64_t)md[2];
  q->scanned_since_fetch = false;
  if (md[1]) return fail(PA_EUNSUPPORTED, "group-key table overflow (more distinct groups than slots)");
  if (md[3]) return fail(PA_EHIP, "internal: partitioned passes disagree on record counts");
  const int64_t m = trim;
  if (m == 0 || capacity < m) return m;

  // the output columns of the kept groups, in pa_query_fetch's staging layout
  FinalDesc f;
  std::memset(&f, 0, sizeof(f));
  f.nagg = s.num_aggs;
  std::vector<size_t> off(s.num_aggs, 0);
  size_t bytes = ((size_t)m * 16 + 255) & ~(size_t)255;  // keys | counts
  for (int a = 0; a < s.num_aggs; ++a) {
    const pa_agg_spec& A = s.aggs[a];
    f.type[a] = A.type;
    f.src[a] = q->hq.aggs[a].src;
    f.sec[a] = q->agg_section[a] >= 0 ? q->sections[q->agg_section[a]].ptr : nullptr;
    f.per[a] = A.type == PA_AGG_DISTINCTCOUNT ? presence_stride(A)
               : (A.type == PA_AGG_DISTINCTCOUNTHLL ? (int64_t(1) << A.log2m) : 8);
    off[a] = bytes;
    bytes += ((size_t)m * (size_t)f.per[a] + 255) & ~(size_t)255;
  }
  if (q->fetch_stage.n < bytes) {
    dev_free(q->fetch_stage);
    if (int rc = dev_alloc(q->fetch_stage, bytes)) return rc;
  }
  char* ds = (char*)q->fetch_stage.p;
  f.keys = (int64_t*)ds;
  f.counts = (int64_t*)(ds + (size_t)m * 8);
  for (int a = 0; a < s.num_aggs; ++a) f.out[a] = ds + off[a];

  // scratch: candidate keys | order words | flags | kept candidates | control | histograms | states
  const int nwords = spec->num_terms + 1;
  const size_t col = ((size_t)n * 8 + 255) & ~(size_t)255;
  const size_t ctl_bytes = (sizeof(TrimCtl) + 255) & ~(size_t)255;
  const size_t hist_bytes = (size_t)kTrimMaxPasses * 256 * 4;
  const size_t need = col * (size_t)(nwords + 3) + ctl_bytes + hist_bytes + (size_t)n;
  if (q->trim_buf.n < need) {
    dev_free(q->trim_buf);
    if (int rc = dev_alloc(q->trim_buf, need)) return rc;
  }
  char* tb = (char*)q->trim_buf.p;
  int64_t* cand = (int64_t*)tb;
  w.words = (uint64_t*)(tb + col);
  TrimPlan p;
  std::memset(&p, 0, sizeof(p));
  p.n = n;
  p.words = w.words;
  p.flag = (unsigned long long*)(tb + col * (size_t)(nwords + 1));
  int64_t* sel = (int64_t*)(tb + col * (size_t)(nwords + 2));
  p.ctl = (TrimCtl*)(tb + col * (size_t)(nwords + 3));
  p.hist = (uint32_t*)((char*)p.ctl + ctl_bytes);
  p.state = (uint8_t*)p.hist + hist_bytes;
  // digit passes, most significant first: a key column's id and the tie word are below their cardinality / the key
  // count, so their high bytes are the same in every candidate
  for (int e = 0; e < nwords; ++e) {
    int nbytes = 8;
    if (e == spec->num_terms) nbytes = bytes_below((uint64_t)K);
    else if (spec->kind[e] == PA_TRIM_KEY_COLUMN) nbytes = bytes_below((uint64_t)w.kcard[e]);
    for (int b = nbytes - 1; b >= 0; --b) {
      p.word[p.npass] = e;
      p.shift[p.npass] = 8 * b;
      ++p.npass;
    }
  }
  CompactDesc d;
  std::memset(&d, 0, sizeof(d));
  d.keys = cand;
  PA_HIP(launch_compact(count, K, all, blocks, n, &d, 1, st));
  PA_HIP(launch_trim_words(count, &f, &w, cand, n, st));
  PA_HIP(launch_trim_select(&p, m, st));
  // the kept candidates in ascending order: the same count + scan + gather over the flags (n <= K: the block sums fit)
  const int64_t nb2 = (n + 2047) / 2048;
  d.keys = sel;
  PA_HIP(launch_compact(p.flag, n, 0, blocks, 0, nullptr, 0, st));
  PA_HIP(launch_compact(p.flag, n, 0, blocks, m, &d, 1, st));
  PA_HIP(launch_trim_rows(count, cand, sel, n, m, &f, st));
  uint32_t kept = 0;
  PA_HIP(hipMemcpyAsync(&kept, blocks + nb2, 4, hipMemcpyDeviceToHost, st));
  if (out_keys) PA_HIP(hipMemcpyAsync(out_keys, f.keys, (size_t)m * 8, hipMemcpyDeviceToHost, st));
  if (out_counts) PA_HIP(hipMemcpyAsync(out_counts, f.counts, (size_t)m * 8, hipMemcpyDeviceToHost, st));
  for (int a = 0; a < s.num_aggs; ++a)
    if (out_aggs && out_aggs[a])
      PA_HIP(hipMemcpyAsync(out_aggs[a], f.out[a], (size_t)m * (size_t)f.per[a], hipMemcpyDeviceToHost, st));
  PA_HIP(hipStreamSynchronize(st));
  if ((int64_t)kept != m) return fail(PA_EHIP, "internal: the group trim kept a wrong number of groups");
  return m;
}

// The row layout of a hashed block: every per-key section (numDocsScanned counters excluded) in section order.
static int row_desc(const pa_query* q, RowDesc& d) {
  if (!q || !q->prepared) return fail(PA_EINVAL, "query not prepared");
  if (!q->hashed || q->keys_section < 0) return fail(PA_EINVAL, "row merge needs a hashed key space");
  std::memset(&d, 0, sizeof(d));
  int64_t off = 0;
  for (const Section& sc : q->sections) {
    if (sc.kind == PA_ACC_DOCS_U64) continue;
    if (d.nsec >= kMaxRowSecs) return fail(PA_EINVAL, "internal: too many sections for a row");
    RowSec& r = d.sec[d.nsec++];
    switch (sc.kind) {
      case PA_ACC_SUM_F64: r.op = ROW_ADD_F64; break;
      case PA_ACC_MIN_I64: r.op = ROW_MIN_I64; break;
      case PA_ACC_MAX_I64: r.op = ROW_MAX_I64; break;
      case PA_ACC_HLL_U8: case PA_ACC_PRESENCE_U8: r.op = ROW_MAX_U8; break;
      case PA_ACC_KEYS_I64: r.op = ROW_KEY; break;
      default: r.op = ROW_ADD_U64; break;  // COUNT, SUM (int64 and the exact lo / hi pair)
    }
    r.slot_bytes = sc.n / q->num_keys * (int64_t)section_es(sc.kind);
    if (r.slot_bytes % 8) return fail(PA_EINVAL, "internal: row section not a multiple of 8 bytes");
    r.row_off = off;
    r.base = sc.ptr;
    if (sc.kind == PA_ACC_KEYS_I64) {
      d.key_off = off;
      d.keys = (long long*)sc.ptr;
    }
    if (sc.kind == PA_ACC_COUNT_U64) d.count = (const unsigned long long*)sc.ptr;
    off += r.slot_bytes;
  }
  d.row_bytes = off;
  d.num_slots = q->num_keys;
  d.ht_mask = q->ht_slots - 1;
  d.key_words = q->key_words;
  return PA_OK;
}

static int merge_scratch(pa_query* q, size_t bytes) {
  if (q->merge_buf.n >= bytes) return PA_OK;
  dev_free(q->merge_buf);
  return dev_alloc(q->merge_buf, bytes);
}

int64_t pa_query_row_bytes(const pa_query* q) {
  RowDesc d;
  const int rc = row_desc(q, d);
  return rc ? rc : d.row_bytes;
}

int pa_query_pack_rows(pa_query* q, int32_t world, void* device_rows, int64_t* counts, void* stream) {
  RowDesc d;
  int rc = row_desc(q, d);
  if (!rc) rc = refuse_invalid(q);
  if (rc) return rc;
  if (world < 1|| world > 1024 || !counts) return fail(PA_EINVAL, "pack rows: bad world size or null counts");
  hipStream_t st = (hipStream_t)stream;
  // scratch: counts[world], cursor[world], row_slot[num_slots]
  rc = merge_scratch(q, (size_t)(2 * world + d.num_slots) * 8);
  if (rc) return rc;
  unsigned long long* cnt = (unsigned long long*)q->merge_buf.p;
  unsigned long long* cur = cnt + world;
  int64_t* row_slot = (int64_t*)(cur + world);
  PA_HIP(hipMemsetAsync(cnt, 0, (size_t)world * 8, st));
  PA_HIP(launch_pack_index(d, world, 0, cnt, nullptr, nullptr, st));
  std::vector<unsigned long long> h(world);
  PA_HIP(hipMemcpyAsync(h.data(), cnt, (size_t)world * 8, hipMemcpyDeviceToHost, st));
  PA_HIP(hipStreamSynchronize(st));
  int64_t total = 0;
  std::vector<unsigned long long> start(world);
  for (int r = 0; r < world; ++r) {
    counts[r] = (int64_t)h[r];
    start[r] = (unsigned long long)total;
    total += (int64_t)h[r];
  }
  if (!device_rows || total == 0) return PA_OK;
  PA_HIP(hipMemcpyAsync(cur, start.data(), (size_t)world * 8, hipMemcpyHostToDevice, st));
  PA_HIP(launch_pack_index(d, world, 1, nullptr, cur, row_slot, st));
  PA_HIP(launch_pack_copy(d, row_slot, total, (unsigned char*)device_rows, st));
  PA_HIP(hipStreamSynchronize(st));
  return PA_OK;
}

int pa_query_merge_rows(pa_query* q, const void* device_rows, int64_t num_rows, int64_t* groups, int64_t* overflow,
                        void* stream) {
  RowDesc d;
  int rc = row_desc(q, d);
  if (!rc) rc = refuse_invalid(q);
  if (rc) return rc;
  if (num_rows < 0|| (num_rows > 0 && !device_rows)) return fail(PA_EINVAL, "merge rows: bad rows");
  hipStream_t st = (hipStream_t)stream;
  rc = merge_scratch(q, (size_t)(8 + std::max<int64_t>(num_rows, d.num_slots)) * 8);
  if (rc) return rc;
  unsigned long long* ctr = (unsigned long long*)q->merge_buf.p;
  int64_t* row_slot = (int64_t*)(ctr + 8);
  // the block is reset except its numDocsScanned counters, which stay this rank's (the broker sums them)
  void* docs = q->sections.back().ptr;
  PA_HIP(hipMemcpyAsync(ctr + 4, docs, 32, hipMemcpyDeviceToDevice, st));
  rc = pa_query_reset(q, stream);
  if (rc) return rc;
  PA_HIP(hipMemcpyAsync(docs, ctr + 4, 32, hipMemcpyDeviceToDevice, st));
  PA_HIP(hipMemsetAsync(ctr, 0, 32, st));
  PA_HIP(launch_merge_rows(d, (const unsigned char*)device_rows, num_rows, row_slot, ctr, st));
  unsigned long long h[4];
  PA_HIP(hipMemcpyAsync(h, ctr, 32, hipMemcpyDeviceToHost, st));
  PA_HIP(hipStreamSynchronize(st));
  if (groups) *groups = (int64_t)h[0];
  if (overflow) *overflow = (int64_t)h[1];
  return PA_OK;
}

}  // extern "C"
