// Host side of the C-ABI (include/pinot_amd.h): segment residency, query planning (CNF filter, column
// slots, staging, accumulator layout, strategy) and result fetch. No CPU fallback: every query runs the
// HIP kernels; errors surface as negative return codes + pa_last_error().
#include "pa_host.h"

extern "C" {

pa_query* pa_query_create(const pa_query_spec* spec, int32_t num_segments) {
  if (!spec || num_segments < 0) {
    fail(PA_EINVAL, "bad query spec");
    return nullptr;
  }
  if (spec->num_leaves < 0 || spec->num_leaves > PA_MAX_LEAVES || spec->num_ops < 0 || spec->num_ops > PA_MAX_OPS ||
      spec->num_group_by < 0 || spec->num_group_by > PA_MAX_GROUP_BY || spec->num_aggs < 0 ||
      spec->num_aggs > PA_MAX_AGGS) {
    fail(PA_EINVAL, "query spec counts out of range");
    return nullptr;
  }
  pa_query* q = new pa_query();
  q->spec = *spec;
  q->nseg = num_segments;
  q->segs.assign(num_segments, nullptr);
  q->leaf_params.resize(num_segments);
  q->luts.resize(num_segments);
  q->remaps.resize(num_segments);
  q->has_remap.resize(num_segments);
  q->vremaps.assign(num_segments, std::vector<std::vector<int32_t>>(spec->num_aggs));
  return q;
}

int pa_query_set_tuning(pa_query* q, const char* name, int32_t value) {
  if (!q) return fail(PA_EINVAL, "null query");
  if (q->prepared) return fail(PA_EINVAL, "query already prepared");
  const TuningDef* d = tuning_named(name);
  if (!d) return fail(PA_EINVAL, std::string("unknown tuning: ") + (name ? name : "(null)"));
  if (value != d->def && (value < d->lo || value > d->hi))
    return fail(PA_EINVAL, std::string("tuning ") + d->name + ": " + std::to_string(value) + " outside " +
                               std::to_string(d->lo) + ".." + std::to_string(d->hi));
  q->tune.*d->value = value;
  return PA_OK;
}

int32_t pa_query_results_invalid(const pa_query* q) { return q ? (tuning_invalidating(q->tune) ? 1 : 0) : -1; }

int pa_query_set_agg_filters(pa_query* q, const pa_agg_filter_spec* spec) {
  if (!q || !spec) return fail(PA_EINVAL, "null query or aggregation-filter spec");
  if (q->prepared) return fail(PA_EINVAL, "query already prepared");
  for (const pa_segment* seg : q->segs)
    if (seg) return fail(PA_EINVAL, "set the aggregation filters before binding segments");
  if (q->is_select || q->is_distinct) return fail(PA_EINVAL, "aggregation filters on a selection or distinct query");
  if (q->is_expr) return fail(PA_EUNSUPPORTED, "aggregation filters next to expressions are not supported");
  const pa_query_spec& s = q->spec;
  if (spec->num_filters < 1 || spec->num_filters > PA_MAX_AGG_FILTERS)
    return fail(PA_EINVAL, "aggregation filters: 1.." + std::to_string(PA_MAX_AGG_FILTERS) + " filters");
  std::vector<char> used(spec->num_filters, 0);
  for (int a = 0; a < s.num_aggs; ++a) {
    const int f = spec->agg_filter[a];
    if (f < -1 || f >= spec->num_filters) return fail(PA_EINVAL, "aggregation filter index out of range");
    if (f >= 0) used[f] = 1;
  }
  std::vector<std::vector<Literal>> lits(spec->num_filters);
  std::vector<std::vector<int>> ends(spec->num_filters);
  size_t total = 0;
  for (int f = 0; f < spec->num_filters; ++f) {
    if (!used[f]) return fail(PA_EINVAL, "an aggregation filter no aggregation uses");
    if (spec->num_ops[f] < 1 || spec->num_ops[f] > PA_MAX_OPS) return fail(PA_EINVAL, "aggregation filter: bad program length");
    std::vector<Clause> cnf;
    if (int rc = to_cnf_program(spec->ops[f], spec->num_ops[f], s.num_leaves, cnf)) return rc;
    for (const Clause& c : cnf)
      for (size_t i = 0; i < c.size(); ++i) {
        lits[f].push_back(c[i]);
        ends[f].push_back(i + 1 == c.size());
      }
    total += lits[f].size();
  }
  if (total > PA_MAX_LEAVES)
    return fail(PA_EUNSUPPORTED, "aggregation filters expand to more than PA_MAX_LEAVES CNF literals");
  q->filt_spec = *spec;
  q->filt_lits = lits;
  q->filt_clause_end = ends;
  q->is_filtered = true;
  return PA_OK;
}

int pa_query_set_expressions(pa_query* q, const pa_expr_spec* spec) {
  if (!q || !spec) return fail(PA_EINVAL, "null query or expression spec");
  if (q->prepared) return fail(PA_EINVAL, "query already prepared");
  // (the spec's columns at the expressions' positions are rewritten below, and a bind reads them)
  for (const pa_segment* seg : q->segs)
    if (seg) return fail(PA_EINVAL, "set the expressions before binding segments");
  if (q->is_select || q->is_distinct) return fail(PA_EINVAL, "expressions on a selection or distinct query");
  if (q->is_filtered) return fail(PA_EUNSUPPORTED, "expressions next to aggregation filters are not supported");
  if (int rc = expr_check_spec(q->spec, *spec)) return rc;
  q->expr_spec = *spec;
  q->is_expr = true;
  // The spec's column at an expression's position is ignored: it becomes the program's first operand column, so every
  // per-column step of the planner sees a column the query really reads.
  auto first_col = [&](int e) {
    const pa_expr_program& p = spec->exprs[e];
    for (int o = 0; o < p.num_ops; ++o)
      if (p.ops[o].op == PA_EXPR_LOAD_COL) return spec->columns[p.ops[o].a];
    return spec->columns[0];
  };
  for (int a = 0; a < q->spec.num_aggs; ++a)
    if (spec->agg_expr[a] >= 0) q->spec.aggs[a].column_id = first_col(spec->agg_expr[a]);
  for (int j = 0; j < q->spec.num_group_by; ++j)
    if (spec->group_by_expr[j] >= 0) {
      q->spec.group_by_columns[j] = first_col(spec->group_by_expr[j]);
      q->spec.group_by_cardinality[j] = 0;
    }
  return PA_OK;
}

int pa_query_set_moments(pa_query* q, const pa_moments_spec* spec) {
  if (!q || !spec) return fail(PA_EINVAL, "null query or moments spec");
  if (q->prepared) return fail(PA_EINVAL, "query already prepared");
  if (q->is_select || q->is_distinct) return fail(PA_EINVAL, "moments on a selection or distinct query");
  for (int a = 0; a < q->spec.num_aggs; ++a) {
    if (q->spec.aggs[a].type != PA_AGG_MOMENTS) continue;
    if (spec->form[a] < PA_MOMENTS_FORM_AUTO || spec->form[a] > PA_MOMENTS_FORM_DOUBLE)
      return fail(PA_EINVAL, "moments: bad form");
    if (spec->has_pivot[a] && !std::isfinite(spec->pivot[a])) return fail(PA_EINVAL, "moments: the pivot must be finite");
    if (spec->has_pivot[a] && spec->second_column[a] >= 0) return fail(PA_EINVAL, "moments: a covariance takes no pivot");
  }
  q->mom_spec = *spec;
  q->mom_spec_set = true;
  return PA_OK;
}

int pa_query_moments_form(const pa_query* q, int32_t agg, int32_t* out_form, double* out_pivot) {
  if (!q || !q->prepared || agg < 0 || agg >= q->spec.num_aggs || !q->mom_form[agg])
    return fail(PA_EINVAL, "not a prepared PA_AGG_MOMENTS aggregation");
  if (out_form) *out_form = q->mom_form[agg];
  if (out_pivot) *out_pivot = q->mom_pivot[agg];
  return PA_OK;
}

int pa_query_lane_docs(pa_query* q, int64_t* out) {
  if (!q || !q->prepared || !out) return fail(PA_EINVAL, "query not prepared");
  if (!q->is_filtered) return fail(PA_EINVAL, "not a query with aggregation filters");
  const size_t n = (size_t)q->nseg * (q->filt_spec.num_filters + 1);
  if (!q->scanned_since_fetch && q->last_matched >= 0 && q->filt_seg_docs_host.size() == n) {
    // the last pa_query_fetch read the counters with its own copy, after the last scan: no second synchronisation
    std::copy(q->filt_seg_docs_host.begin(), q->filt_seg_docs_host.end(), out);
    return PA_OK;
  }
  PA_HIP(hipDeviceSynchronize());
  PA_HIP(hipMemcpy(out, q->filt_seg_docs.p, n * 8, hipMemcpyDeviceToHost));
  return PA_OK;
}

int pa_query_bind_segment(pa_query* q, int32_t index, const pa_segment* seg, const pa_leaf_params* leaf_params,
                          const int32_t* const* group_remaps) {
  if (!q || !seg || index < 0 || index >= q->nseg) return fail(PA_EINVAL, "bad bind arguments");
  if (q->prepared) return fail(PA_EINVAL, "query already prepared");
  const pa_query_spec& s = q->spec;
  q->segs[index] = seg;
  q->leaf_params[index].assign(leaf_params, leaf_params + s.num_leaves);
  q->luts[index].assign(s.num_leaves, {});
  for (int l = 0; l < s.num_leaves; ++l) {
    const int kind = s.leaves[l].kind;
    if (kind == PA_LEAF_DICT_SET || kind == PA_LEAF_MV_DICT_SET) {
      auto it = seg->cols.find(s.leaves[l].column_id);
      if (it == seg->cols.end()) return fail(PA_EINVAL, "leaf column missing in segment");
      if (!leaf_params[l].lut) return fail(PA_EINVAL, "DICT_SET leaf without lut");
      const size_t words = ((size_t)it->second->cardinality + 31) / 32;
      q->luts[index][l].assign(leaf_params[l].lut, leaf_params[l].lut + words);
    } else if (kind == PA_LEAF_RAW_SET) {  // (the values, 8 bytes each, kept as word pairs)
      auto it = seg->cols.find(s.leaves[l].column_id);
      if (it == seg->cols.end()) return fail(PA_EINVAL, "leaf column missing in segment");
      const int64_t n = leaf_params[l].num_values;
      if (n < 0 || n > (int64_t(1) << 30) || (n > 0 && !leaf_params[l].values))
        return fail(PA_EINVAL, "RAW_SET leaf: bad value list");
      const bool integral = it->second->vtype == PA_INT || it->second->vtype == PA_LONG;
      const int64_t* vi = (const int64_t*)leaf_params[l].values;
      const double* vd = (const double*)leaf_params[l].values;
      for (int64_t i = 1; i < n; ++i)
        if (integral ? !(vi[i - 1] < vi[i]) : !(vd[i - 1] < vd[i]))
          return fail(PA_EINVAL, "RAW_SET leaf: values must be strictly ascending");
      const uint32_t* w = (const uint32_t*)leaf_params[l].values;
      q->luts[index][l].assign(w, w + 2 * n);
    }
  }
  q->remaps[index].assign(s.num_group_by, {});
  q->has_remap[index].assign(s.num_group_by, 0);
  for (int j = 0; j < s.num_group_by; ++j) {
    if (group_remaps && group_remaps[j]) {
      auto it = seg->cols.find(s.group_by_columns[j]);
      if (it == seg->cols.end()) return fail(PA_EINVAL, "group-by column missing in segment");
      const int32_t card = it->second->cardinality;
      q->remaps[index][j].assign(group_remaps[j], group_remaps[j] + card);
      for (int32_t v : q->remaps[index][j])
        if (v < 0 || v >= s.group_by_cardinality[j]) return fail(PA_EINVAL, "group remap id outside the key space");
      q->has_remap[index][j] = 1;
    }
  }
  return PA_OK;
}

int pa_query_bind_value_remap(pa_query* q, int32_t index, int32_t agg, const int32_t* remap) {
  if (!q || index < 0 || index >= q->nseg || agg < 0 || agg >= q->spec.num_aggs) return fail(PA_EINVAL, "bad remap arguments");
  if (q->prepared) return fail(PA_EINVAL, "query already prepared");
  if (!q->segs[index]) return fail(PA_EINVAL, "bind the segment before its value remaps");
  const pa_agg_spec& A = q->spec.aggs[agg];
  if (!value_id_agg(A.type) && !time_row_agg(A.type))
    return fail(PA_EINVAL, "value remaps belong to DISTINCTCOUNT, VALUE_HISTOGRAM and LAST / FIRST_ROW_BY_TIME aggregations");
  auto it = q->segs[index]->cols.find(A.column_id);
  if (it == q->segs[index]->cols.end()) return fail(PA_EINVAL, "aggregation column missing in segment");
  if (time_row_agg(A.type) && it->second->kind != COL_SV_DICT)
    return fail(PA_EINVAL, "a value remap for a time column that is not dictionary-encoded in this segment");
  q->vremaps[index][agg].clear();
  if (!remap) return PA_OK;
  const int32_t card = it->second->cardinality;
  q->vremaps[index][agg].assign(remap, remap + card);
  for (int32_t v : q->vremaps[index][agg])
    if (v < 0 || v >= A.num_values) return fail(PA_EINVAL, "value remap id outside the table-wide value dictionary");
  return PA_OK;
}

int pa_query_prepare(pa_query* q) {
  if (!q) return fail(PA_EINVAL, "null query");
  if (q->prepared) return PA_OK;
  for (int i = 0; i < q->nseg; ++i)
    if (!q->segs[i]) return fail(PA_EINVAL, "segment " + std::to_string(i) + " not bound");
  Prep P;
  std::memset(&q->hq, 0, sizeof(q->hq));
  int rc = q->is_select ? select_validate(q) : PA_OK;
  if (!rc) rc = plan_filter(q, P);
  if (!rc) rc = plan_slots(q, P);
  if (!rc) rc = plan_key_space(q, P);
  if (!rc) rc = plan_limit(q, P);
  // (a distinct query and a query with aggregation filters have their own two strategies each)
  if (!rc && !q->is_distinct && !q->is_filtered && !q->is_expr && !q->is_trow && !q->is_moments) rc = plan_gdense(q, P);
  if (!rc) rc = build_segments(q, P);
  if (!rc && q->is_filtered) rc = filtered_validate(q, P);
  if (!rc && q->is_expr) rc = expr_validate(q, P);
  if (!rc) rc = trow_validate(q, P);
  if (!rc) rc = mom_validate(q, P);
  if (!rc) rc = plan_walk(q, P);
  if (!rc) rc = plan_accumulators(q, P);
  TilePlan plan, count_plan;
  if (!rc) rc = plan_kernels(q, P, plan, count_plan);
  if (rc) return rc;

  // layout: tiles per segment, LDS regions (the count pass has its own staging), staged bytes
  void* dummy = nullptr;  // 256 readable bytes: source of the DMA padding instructions
  {
    std::vector<char> z(256, 0);
    rc = upload_owned(q, z.data(), z.size(), &dummy);
    if (rc) return rc;
  }
  const int nslots = (int)q->slot_cols.size();
  int64_t total_tiles = 0;
  apply_layout(q->hsegs, plan.steps, nslots, (int)q->literals.size(), dummy, &q->staged_bytes, &total_tiles);
  q->num_tiles = (uint64_t)total_tiles;
  q->lane_major = P.lm ? 1 : 0;
  q->dense_packed = P.gd_packed ? 1 : 0;
  q->plan_ring = plan.ring;
  q->plan_wg = plan.wg_per_cu;
  fill_devquery(q, P, plan, total_tiles);
  if (q->is_filtered) {
    rc = filtered_plan(q, P);
    if (rc) return rc;
  }
  if (q->is_expr) {
    rc = expr_plan(q, P);
    if (rc) return rc;
  }
  if (q->is_trow) {
    rc = trow_plan(q);
    if (rc) return rc;
  }
  if (q->is_moments) {
    rc = mom_plan(q);
    if (rc) return rc;
  }
  rc = plan_leaps(q, P);
  if (rc) return rc;

  // grid: persistent waves, enough workgroups to cover the CUs several times over
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
  }
  const int wg_cu = q->split_emit ? std::min(plan.wg_per_cu, q->emit_h_wg) : plan.wg_per_cu;
  const int64_t max_wg = (int64_t)cus * std::max(1, wg_cu);
  const int wpw = q->partitioned ? scan_waves(q->emit_strat) : scan_waves(q->strategy);
  const int64_t want = (total_tiles + wpw - 1) / wpw;
  q->grid = (int)std::max<int64_t>(1, std::min(max_wg, want));
  if (q->tune.scan_grid > 0 && !q->partitioned) q->grid = (int)std::min<int64_t>(q->grid, q->tune.scan_grid);
  if (q->is_select) {  // (may shrink the grid: every wave owns a candidate segment of the scratch block)
    rc = select_plan(q);
    if (rc) return rc;
  }

  if (q->partitioned) {
    // the count pass: the same tiles, waves and grid; only the group-by and filter columns staged
    int64_t ct = 0;
    apply_layout(q->hsegs_count, plan.steps, nslots, (int)q->literals.size(), dummy, nullptr, &ct);
    if (ct != total_tiles) return fail(PA_EINVAL, "internal: count pass tiles differ");
    DevQuery& c = q->hq_count;
    c = q->hq;
    c.strategy = q->count_strat;
    c.count_skip_gb = q->count_skip;
    c.image_dwords_max = count_plan.img_dw;
    c.ring = count_plan.ring;
    c.dma_per_tile = count_plan.dma;
    c.num_staged = 0;
    for (int sl = 0; sl < nslots; ++sl) {
      bool st = false;
      for (const DevSeg& d : q->hsegs_count) st |= d.cols[sl].lds_off >= 0;
      if (st) c.staged_slots[c.num_staged++] = sl;
    }
    c.lds_acc_bytes = (uint32_t)(((size_t)q->hq.num_parts * 4 + 15) & ~(size_t)15);
    q->count_lds = (int)count_plan.lds;
    q->count_ring = count_plan.ring;
    // the count pass stages fewer columns, so more of its workgroups fit a CU: k per emit workgroup (each walks 1/k of
    // that workgroup's tiles; part_scan_kernel sums their rows), as many as are resident at once
    q->count_k = std::max(1, count_plan.wg_per_cu / std::max(1, wg_cu));
    while (q->count_k > 1 && (int64_t)q->grid * q->count_k * kWavesPerWG > total_tiles) --q->count_k;
    // the emit pass's LDS: partition bin state + bins in front of the ring
    q->hq.lds_acc_bytes = (uint32_t)(plan.lds - (size_t)wpw * plan.ring * plan.img_dw * 4);
    if (q->split_emit) {  // the H launch: same tiles and staging, its own ring depth, bins and partitions
      DevQuery& e = q->hq_h;
      e = q->hq;
      e.strategy = STRAT_PEMIT;
      e.ring = q->emit_h_ring;
      e.lds_acc_bytes = (uint32_t)((size_t)q->emit_h_lds -
                                   (size_t)scan_waves(q->emit_h_strat) * q->emit_h_ring * plan.img_dw * 4);
      e.part_lo = q->hq.pv;
      e.part_hi = q->hq.num_parts;
    }
    rc = plan_scratch(q, P);
    if (rc) return rc;
  }
  if (q->limit_mode) {
    rc = plan_limit_buffers(q, P, cus, total_tiles);
    if (rc) return rc;
  }
  rc = alloc_leaps(q, P);
  if (rc) return rc;
  rc = upload_descriptors(q);
  if (rc) return rc;
  if (q->trow_wide) {  // the second launch's descriptor: the same query, trow_pass = 2
    rc = dev_alloc(q->dq_pass2, sizeof(DevQuery));
    if (rc) return rc;
    DevQuery h2 = q->hq;
    h2.trow_pass = 2;
    PA_HIP(hipMemcpy(q->dq_pass2.p, &h2, sizeof(DevQuery), hipMemcpyHostToDevice));
  }
  if (!q->is_distinct) rc = jit_plan(q, P, cus);
  if (!rc) rc = eqs_plan(q, P, cus);
  if (rc) return rc;
  if (q->is_distinct) {
    rc = distinct_plan(q);
    if (rc) return rc;
  }
  rc = pve_plan(q, P, cus);
  if (rc) return rc;
  PA_HIP(hipDeviceSynchronize());
  q->prepared = true;
  return PA_OK;
}

int64_t pa_query_num_keys(const pa_query* q) { return q ? q->num_keys : -1; }

int pa_query_reset(pa_query* q, void* stream) {
  if (!q || !q->prepared) return fail(PA_EINVAL, "query not prepared");
  hipStream_t st = (hipStream_t)stream;
  char* block = (char*)(q->external_acc ? q->external_acc : q->acc.p);
  if (q->is_select)
    if (int rc = select_reset(q, st)) return rc;
  // (the lane counts lie in the block: identity 0, like every SUM section; the per-segment doc counters do not)
  if (q->is_filtered) PA_HIP(hipMemsetAsync(q->filt_seg_docs.p, 0, q->filt_seg_docs.n, st));
  // Small blocks (the common case): one launch writes zeros and identities (the block is whole 256-byte units). Larger
  // ones keep the memsets, whose rate matters there and whose extra launches no longer do.
  auto identity = [](const Section& sc, int64_t& v) {
    if (sc.kind == PA_ACC_MIN_I64 || sc.kind == PA_ACC_KEYS_I64) v = INT64_MAX;
    else if (sc.kind == PA_ACC_MAX_I64 || sc.kind == PA_ACC_TIME_MAX_I64) v = INT64_MIN;
    else return false;
    return true;
  };
  const bool fused = q->tune.reset_fused < 0 ? q->acc.n <= kResetFusedMaxBytes : q->tune.reset_fused != 0;
  if (fused) {
    ResetArgs a{};
    a.block = (int64_t*)block;
    a.block_words = (int64_t)(q->acc.n / 8);
    if (q->hq.leap_mode) {
      a.header = (int64_t*)q->leap_buf.p;
      a.header_words = (int64_t)(leap_header_bytes(q) / 8);
    }
    bool fits = true;
    for (const Section& sc : q->sections) {
      int64_t v;
      if (!identity(sc, v)) continue;
      if (a.num_sections == ResetArgs::kMaxSections) {
        fits = false;
        break;
      }
      a.sec[a.num_sections].first = ((char*)sc.ptr - block) / 8;
      a.sec[a.num_sections].n = sc.n;
      a.sec[a.num_sections].value = v;
      ++a.num_sections;
    }
    if (fits) {
      PA_HIP(launch_reset(a, st));
      return PA_OK;
    }
  }
  PA_HIP(hipMemsetAsync(block, 0, q->acc.n, st));
  if (q->hq.leap_mode) PA_HIP(hipMemsetAsync(q->leap_buf.p, 0, leap_header_bytes(q), st));
  for (const Section& sc : q->sections) {
    if (sc.kind == PA_ACC_MIN_I64 || sc.kind == PA_ACC_KEYS_I64) PA_HIP(launch_fill_i64((int64_t*)sc.ptr, sc.n, INT64_MAX, st));
    else if (sc.kind == PA_ACC_MAX_I64 || sc.kind == PA_ACC_TIME_MAX_I64)
      PA_HIP(launch_fill_i64((int64_t*)sc.ptr, sc.n, INT64_MIN, st));
  }
  return PA_OK;
}

int pa_query_scan(pa_query* q, void* stream) {
  if (!q || !q->prepared) return fail(PA_EINVAL, "query not prepared");
  q->scanned_since_fetch = true;
  if (q->num_tiles == 0) return PA_OK;
  hipStream_t st = (hipStream_t)stream;
  if (q->limit_walk) {  // admitted keys of every segment where the limit can bind, before any pass tests them
    if (q->walk_words > kWalkMaxWords) PA_HIP(hipMemsetAsync(q->lim_admit.p, 0, q->lim_admit.n, st));
    PA_HIP(launch_limit_walk((const DevQuery*)q->dq.p, (const DevSeg*)q->dsegs.p, q->nseg, q->walk_words,
                             q->hq.gb_mv >= 0, q->tune.walk_tab != 0, st));
  }
  if (q->limit_mode) {  // first-seen positions, per-segment selection of the threshold, admitted aggregation
    const DevQuery* dq = (const DevQuery*)q->dq.p;
    const DevSeg* ds = (const DevSeg*)q->dsegs.p;
    const LimitDesc& F = q->limit;
    const int64_t H = F.fmask + 1;
    PA_HIP(launch_fill_i64((int64_t*)F.fkeys, H, INT64_MAX, st));
    PA_HIP(launch_fill_i64((int64_t*)F.fpos, H, -1, st));
    PA_HIP(launch_fill_i64((int64_t*)F.thresh, std::max(1, q->nseg), -1, st));
    PA_HIP(launch_fill_i64((int64_t*)F.hist, std::max(1, q->nseg) * 128, 0, st));
    PA_HIP(launch_limit_passes(dq, ds, F, q->limit_grid, 0, st));
    PA_HIP(launch_limit_passes(dq, ds, F, q->limit_grid, 1, st));
    PA_HIP(launch_limit_passes(dq, ds, F, q->limit_grid, 2, st));
    return PA_OK;
  }
  if (q->pve.fn) {  // the count-free emit: records in per-workgroup chunks, the partitions' chunk lists, pass C
    if (q->part_vk == kVkGeneric) return fail(PA_EINVAL, "internal: chunk lists need a specialised pass C");
    PartScratch ps{};
    char* vb = (char*)q->pve.buf.p;
    ps.base = (uint64_t*)(vb + q->pve.o_base);
    for (pa_query::PveStream* S : {&q->pve, &q->pvh}) {
      if (!S->fn) continue;
      void* pa = S->args.p;
      void* psg = S->segs.p;
      void* params[] = {&pa, &psg};
      PA_HIP(hipModuleLaunchKernel(S->fn, S->grid, 1, 1, S->waves * kWave, 1, 1, S->lds, st, params, nullptr));
      char* b = (char*)S->buf.p;
      // (the H partitions' bases follow the V partitions' in the V buffer's base array: base[pv + 1 ..])
      uint64_t* base = S == &q->pve ? ps.base : ps.base + q->hq.pv + 1;
      PA_HIP(launch_pve_lists((const uint32_t*)(b + S->o_hist), (uint32_t*)(b + S->o_off), base,
                              (const uint32_t*)(b + S->o_table), (const uint32_t*)(b + S->o_used),
                              (uint32_t*)(b + S->o_index), (uint32_t*)(b + S->o_tot), S->grid, S->parts, S->chunks,
                              S->cr, st));
      if (S == &q->pve) {
        ps.recs_v = (uint32_t*)b;
        ps.chunk_index = (const uint32_t*)(b + S->o_index);
        ps.chunk_shift = __builtin_ctz((unsigned)S->cr);
        ps.chunk_bin_shift = S->bin_shift;
      } else {
        ps.recs_h = (uint32_t*)b;
        ps.chunk_index_h = (const uint32_t*)(b + S->o_index);
        ps.chunk_shift_h = __builtin_ctz((unsigned)S->cr);
        ps.chunk_bin_shift_h = S->bin_shift;
      }
    }
    PA_HIP(launch_part_agg(q->part_vk, (const DevQuery*)q->dq.p, ps, q->pvh.fn ? q->hq.num_parts : q->hq.pv,
                           q->hq.pv, q->hq.v_fmt <= V_FMT_ID, q->tune.passc_v16, q->part_lds_c, st));
    return PA_OK;
  }
  if (q->partitioned) {  // count pass, range offsets, emit pass into the partitions, per-partition aggregation
    ScratchArena* a = arena_for(q->scratch_dev);
    std::lock_guard<std::mutex> g(a->mu);
    int rc = arena_grow(a, q->sc_bytes);
    if (rc) return rc;
    if (a->used && a->last_stream != st) PA_HIP(hipStreamWaitEvent(st, a->last, 0));
    const PartScratch ps = scratch_of(q, a->p);
    const LmSegPlan* plans = (const LmSegPlan*)q->dplans.p;
    PA_HIP(launch_scan(q->count_strat, q->steps, 0, q->grid * q->count_k, q->count_lds, (const DevQuery*)q->dq_count.p,
                       (const DevSeg*)q->dsegs_count.p, plans, ps, st));
    PA_HIP(launch_part_offsets(&q->hq, ps, q->grid, q->count_k, st));
    PA_HIP(launch_scan(q->emit_strat, q->steps, 0, q->grid, q->lds_bytes, (const DevQuery*)q->dq.p,
                       (const DevSeg*)q->dsegs.p, plans, ps, st));
    if (q->split_emit)
      PA_HIP(launch_scan(q->emit_h_strat, q->steps, 0, q->grid, q->emit_h_lds, (const DevQuery*)q->dq_h.p,
                         (const DevSeg*)q->dsegs.p, plans, ps, st));
    PA_HIP(launch_part_agg(q->part_vk, (const DevQuery*)q->dq.p, ps, q->hq.num_parts, q->hq.pv, q->hq.v_fmt <= V_FMT_ID,
                           q->tune.passc_v16, q->part_lds_c, st));
    PA_HIP(hipEventRecord(a->last, st));
    a->last_stream = st;
    a->used = true;
    return PA_OK;
  }
  if (q->jit_fn) {  // the query-shape specialised kernel: dense GROUP BY, or the direct scan of one equality
    void* pa = q->jit_args.p;
    void* ps = q->jit_segs.p;
    void* params[] = {&pa, &ps};
    PA_HIP(hipModuleLaunchKernel(q->jit_fn, q->jit_grid, 1, 1, q->jit_waves * kWave, 1, 1, q->jit_lds, st, params,
                                 nullptr));
    if (q->eq_jit) q->leap_searched = false;  // (as after the generic scan below)
    return PA_OK;
  }
  PartScratch none{};
  PA_HIP(launch_scan(q->strategy, q->steps, q->lane_major, q->grid, q->lds_bytes, (const DevQuery*)q->dq.p,
                     (const DevSeg*)q->dsegs.p, (const LmSegPlan*)q->dplans.p, none, st));
  // row by time, wide form: the same scan again (stream order: the first launch's time words are final), in which only
  // the docs holding their key's winning time accumulate, and only into the row words
  if (q->trow_wide)
    PA_HIP(launch_scan(q->strategy, q->steps, q->lane_major, q->grid, q->lds_bytes, (const DevQuery*)q->dq_pass2.p,
                       (const DevSeg*)q->dsegs.p, (const LmSegPlan*)q->dplans.p, none, st));
  q->leap_searched = false;  // (the neighbour searches of the listed E docs run when the statistics are asked for)
  return PA_OK;
}

int pa_query_execute(pa_query* q, void* stream) {
  const int rc = pa_query_reset(q, stream);
  return rc ? rc : pa_query_scan(q, stream);
}

uint64_t pa_query_accumulator_bytes(const pa_query* q) { return q ? (uint64_t)q->acc.n : 0; }

int pa_query_set_accumulator_buffer(pa_query* q, void* device_buffer, uint64_t bytes) {
  if (!q || !q->prepared) return fail(PA_EINVAL, "query not prepared");
  if (!device_buffer || bytes < q->acc.n) return fail(PA_EINVAL, "accumulator buffer too small");
  if (((uintptr_t)device_buffer & 255) != 0) return fail(PA_EINVAL, "accumulator buffer must be 256-byte aligned");
  char* old = (char*)(q->external_acc ? q->external_acc : q->acc.p);
  char* nb = (char*)device_buffer;
  for (Section& s : q->sections) s.ptr = nb + ((char*)s.ptr - old);
  // every scan descriptor of the query (the partitioned count pass has its own) points into the new block
  auto relocate = [&](DevQuery& h) {
    h.count = (unsigned long long*)(nb + ((char*)h.count - old));
    h.matched_docs = (unsigned long long*)(nb + ((char*)h.matched_docs - old));
    if (h.keybits) h.keybits = (uint32_t*)(nb + ((char*)h.keybits - old));
    if (q->hashed) h.ht_keys = (long long*)(nb + ((char*)h.ht_keys - old));
    for (int a = 0; a < h.num_aggs; ++a) {
      if (q->agg_section[a] < 0) continue;
      void* p = q->sections[q->agg_section[a]].ptr;
      h.aggs[a].acc_i64 = (int64_t*)p;
      h.aggs[a].acc_f64 = (double*)p;
      h.aggs[a].acc_hll = (uint8_t*)p;
    }
  };
  relocate(q->hq);
  if (q->is_trow) {
    for (int a = 0; a < q->hq.num_aggs; ++a)
      if (q->trow_form[a] == 2) q->htrow.agg[a].time = (int64_t*)q->sections[q->trow_time_section[a]].ptr;
    PA_HIP(hipMemcpy(q->trow_desc.p, &q->htrow, sizeof(TrowDesc), hipMemcpyHostToDevice));
    if (q->trow_wide) {
      DevQuery h2 = q->hq;
      h2.trow_pass = 2;
      PA_HIP(hipMemcpy(q->dq_pass2.p, &h2, sizeof(DevQuery), hipMemcpyHostToDevice));
    }
  }
  if (q->is_filtered) {
    q->hfilt.lane_count = (unsigned long long*)q->sections[q->lane_section].ptr;
    PA_HIP(hipMemcpy(q->filt_desc.p, &q->hfilt, sizeof(FiltDesc), hipMemcpyHostToDevice));
  }
  if (q->limit_mode) q->limit.reached = q->hq.matched_docs + 2;
  PA_HIP(hipMemcpy(q->dq.p, &q->hq, sizeof(DevQuery), hipMemcpyHostToDevice));
  if (q->jit_fn) {
    JitArgs a;
    PA_HIP(hipMemcpy(&a, q->jit_args.p, sizeof(a), hipMemcpyDeviceToHost));
    jit_fill_pointers(q, a);
    PA_HIP(hipMemcpy(q->jit_args.p, &a, sizeof(a), hipMemcpyHostToDevice));
  }
  for (pa_query::PveStream* S : {&q->pve, &q->pvh}) {
    if (!S->fn) continue;
    PveArgs a;
    PA_HIP(hipMemcpy(&a, S->args.p, sizeof(a), hipMemcpyDeviceToHost));
    pve_fill_pointers(*S, q->hq.matched_docs, a);
    PA_HIP(hipMemcpy(S->args.p, &a, sizeof(a), hipMemcpyHostToDevice));
  }
  if (q->partitioned) {
    relocate(q->hq_count);
    PA_HIP(hipMemcpy(q->dq_count.p, &q->hq_count, sizeof(DevQuery), hipMemcpyHostToDevice));
    if (q->split_emit) {
      relocate(q->hq_h);
      PA_HIP(hipMemcpy(q->dq_h.p, &q->hq_h, sizeof(DevQuery), hipMemcpyHostToDevice));
    }
  }
  if (!q->external_acc) {
    const size_t n = q->acc.n;
    dev_free(q->acc);
    q->acc.n = n;
  }
  q->external_acc = device_buffer;
  return PA_OK;
}

int32_t pa_query_num_sections(const pa_query* q) { return q ? (int32_t)q->sections.size() : -1; }

void* pa_query_section(const pa_query* q, int32_t section, int32_t* kind, int64_t* num_elements) {
  if (!q || section < 0 || section >= (int32_t)q->sections.size()) {
    fail(PA_EINVAL, "bad section");
    return nullptr;
  }
  if (kind) *kind = q->sections[section].kind;
  if (num_elements) *num_elements = q->sections[section].n;
  return q->sections[section].ptr;
}

int pa_query_stats(const pa_query* q, uint64_t* staged_bytes, uint64_t* num_docs, uint64_t* num_tiles) {
  if (!q) return fail(PA_EINVAL, "null query");
  if (staged_bytes) *staged_bytes = q->staged_bytes;
  if (num_docs) *num_docs = q->num_docs;
  if (num_tiles) *num_tiles = q->num_tiles;
  return PA_OK;
}

int pa_query_plan(const pa_query* q, int32_t* strategy, int32_t* steps, int32_t* dma_slots, int32_t* ring,
                  int32_t* wg_per_cu, int32_t* grid, int32_t* lds_bytes) {
  if (!q || !q->prepared) return fail(PA_EINVAL, "query not prepared");
  // (the query-shape specialised kernel reports the lane-major dense variant it specialises)
  if (strategy)
    *strategy = q->jit_fn && !q->eq_jit ? (q->jit_waves >= 16 ? STRAT_GDENSE_LM16 : STRAT_GDENSE_LM8)
                          : (q->partitioned ? STRAT_PEMIT : q->strategy);
  if (steps) *steps = q->steps;
  if (dma_slots) *dma_slots = q->dma_slots;
  if (ring) *ring = q->plan_ring;
  if (wg_per_cu) *wg_per_cu = q->plan_wg;
  if (grid) *grid = q->grid;
  if (lds_bytes) *lds_bytes = q->lds_bytes;
  return PA_OK;
}

int32_t pa_query_num_eager_literals(const pa_query* q) { return q && q->prepared ? q->num_eager : -1; }

int32_t pa_query_time_row_form(const pa_query* q, int32_t agg) {
  if (!q || !q->prepared || agg < 0 || agg >= q->spec.num_aggs) return -1;
  return q->trow_form[agg];
}

int32_t pa_query_lane_major(const pa_query* q) { return q && q->prepared ? q->lane_major : -1; }
int32_t pa_query_eq_prefilter(const pa_query* q) { return q && q->prepared ? q->eq_prefilter : -1; }
int32_t pa_query_stream_nt(const pa_query* q) { return q && q->prepared ? q->stream_nt : -1; }
int32_t pa_query_eq_jit(const pa_query* q) { return q && q->prepared ? q->eq_jit : -1; }
int32_t pa_query_count_free_emit(const pa_query* q) { return q && q->prepared ? (q->pve.fn ? (q->pvh.fn ? 2 : 1) : 0) : -1; }
int32_t pa_query_partition_keys(const pa_query* q) {
  if (!q || !q->prepared) return -1;
  if (!q->partitioned || q->hq.pv == 0) return 0;
  return q->hq.part_kr_v ? q->hq.part_kr_v : (int32_t)1 << q->hq.kshift_v;
}
int32_t pa_query_dense_packed(const pa_query* q) {
  return q && q->prepared ? (q->jit_fn && !q->eq_jit ? 2 : (q->dense_packed ? 1 : 0)) : -1;
}

int32_t pa_query_column_staged(const pa_query* q, int32_t column_id) {
  if (!q || !q->prepared || q->nseg == 0) return -1;
  for (size_t sl = 0; sl < q->slot_cols.size(); ++sl)
    if (q->slot_cols[sl] == column_id) {
      if (q->jit_fn) return std::count(q->jit_cols.begin(), q->jit_cols.end(), (int)sl) ? 1 : 0;
      return q->hsegs[0].cols[sl].lds_off >= 0 ? 1 : 0;
    }
  return -1;
}

int64_t pa_query_matched_docs(const pa_query* q) { return q && q->prepared ? q->last_matched : -1; }

// ---------------------------------------------------------------- cross-GPU merge of hashed key spaces
int32_t pa_query_limit_trimming(const pa_query* q) {
  return q && q->prepared ? (q->limit_mode ? 1 : (q->limit_walk ? 2 : 0)) : -1;
}

int64_t pa_query_num_groups_limit_reached(const pa_query* q) { return q && q->prepared ? q->last_reached : -1; }

int pa_query_key_layout(const pa_query* q, int32_t* hashed, int32_t* shifts) {
  if (!q || !q->prepared) return fail(PA_EINVAL, "query not prepared");
  if (hashed) *hashed = q->hashed ? 1 : 0;
  if (shifts)
    for (int j = 0; j < q->spec.num_group_by; ++j) shifts[j] = q->hashed ? q->key_shift[j] : 0;
  return PA_OK;
}

int32_t pa_query_key_words(const pa_query* q) { return q && q->prepared ? (q->hashed ? q->key_words : 1) : -1; }

void pa_query_destroy(pa_query* q) { delete q; }

}  // extern "C"
