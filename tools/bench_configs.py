"""Secondary measurements for BASELINE.json configs[2] and configs[4] (the headline configs[1] line is bench.py).

  highcard : configs[2] — GROUP BY 2 dictionary dims (1024 x 1024 = ~1M groups) with SUM/MIN/MAX over every doc
             (and over a 10 % filter); the key space does not fit LDS, so accumulators are global
  star     : configs[4] shape on one GPU — raw DOUBLE SUM + DISTINCTCOUNTHLLMV over a multi-value column, 4-dim
             GROUP BY
  selection: configs[1]'s table — SELECT impressions, clicks ... WHERE (the 10 % filter of bench.py's secondary line)
             ORDER BY clicks DESC LIMIT 10 (selection_topk: the fused filter + top-K scan), and beside it
             SELECT MAX(clicks) with the same WHERE (max_same_where: the same bytes through the lane kernels)

  distinct : SELECT DISTINCT as the key-presence bitmap scan against GROUP BY COUNT(*) of the same columns and WHERE:
             (a) configs[1]'s table, DISTINCT daysSinceEpoch under the 10 % filter (LDS bitmap); (b) configs[2]'s table,
             DISTINCT d1, d2 over every doc (1024 x 1024 keys), as the planner runs it and with distinct_lds = 0

  trim     : configs[2]'s table and GROUP BY with ORDER BY SUM(m) DESC LIMIT 10: (a) the full fetch plus
             reduce.server_trim on the host against (b) the trimmed fetch (pa_query_fetch_trimmed) on the same executor

python tools/bench_configs.py [--workload highcard|star|selection|distinct|trim|all] [--segments S] [--docs D] [--reps R]
Prints one JSON line per (workload, plan): scan-kernel ms per launch (HIP events around back-to-back launches on
the launch stream), rows/s, forward-index bytes staged per launch and GB/s, fetch ms, groups.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def sv_spec(rng, docs, card, dtype="INT", base=0):
    from pinot_amd.segment import num_bits_per_value, pack_bits
    nb = num_bits_per_value(card - 1)
    if card == 1 << nb:  # uniform dictIds over [0, 2^nb) == uniformly random bytes
        fwd = np.frombuffer(rng.bytes((docs * nb + 7) // 8), dtype=np.uint8)
    else:
        fwd = pack_bits(rng.integers(0, card, size=docs).astype(np.uint32), nb)
    return (dtype, np.arange(card, dtype=np.int64) + base, fwd)


def highcard_segment(seed, docs):
    from pinot_amd.segment import segment_from_dict_ids
    rng = np.random.default_rng(seed)
    return segment_from_dict_ids("hc%d" % seed, docs, {
        "d1": sv_spec(rng, docs, 1024, base=1000), "d2": sv_spec(rng, docs, 1024, base=5000),
        "m": sv_spec(rng, docs, 1 << 16, "LONG")})


def highcard_own_segment(seed, docs):
    """configs[2] where every segment built its own dictionaries (SegmentDictionaryCreator.java:104): d1 / d2 runs of 1024
    values starting at a per-segment shift (0..7) of the table-wide 1031-value dictionaries (~1.06M keys), m 65536
    values from a per-segment offset (the table-wide value dictionary is their union)."""
    from pinot_amd.segment import segment_from_dict_ids
    rng = np.random.default_rng(seed)
    return segment_from_dict_ids("hco%d" % seed, docs, {
        "d1": sv_spec(rng, docs, 1024, base=1000 + seed % 8), "d2": sv_spec(rng, docs, 1024, base=5000 + (3 * seed) % 8),
        "m": sv_spec(rng, docs, 1 << 16, "LONG", base=(611 * seed) % 4096)})


def highcard_rd_segment(seed, docs):
    """configs[2] with a non-arithmetic value dictionary: m's 65536 values are sorted random distinct longs, so pass C
    looks every SUM value up in the dictionary (the affine shortcut does not apply)."""
    seg = highcard_segment(seed, docs)
    rng = np.random.default_rng(10_000 + seed)
    vals = np.unique(rng.integers(0, 1 << 40, size=70_000))[:1 << 16]
    assert len(vals) == 1 << 16
    seg.columns["m"].dictionary = np.sort(vals).astype(np.int64)
    return seg


def sumscan_segment(seed, docs):
    """configs[0]: a fixed-bit dictionary-encoded INT dimension (daysSinceEpoch, 1024 days = 10 bits) and a LONG metric
    m whose 16384 dictionary values (14 bits) are sorted random longs below 2^29 (no arithmetic shortcut: every SUM value
    is a dictionary lookup; a 10M-doc segment's sum stays below 2^53, where the reference's double accumulation is
    exact)."""
    from pinot_amd.segment import segment_from_dict_ids
    rng = np.random.default_rng(seed)
    vals = np.unique(np.random.default_rng(777).integers(0, 1 << 29, size=20_000))[:1 << 14].astype(np.int64)
    assert len(vals) == 1 << 14
    return segment_from_dict_ids("ss%d" % seed, docs, {
        "daysSinceEpoch": sv_spec(rng, docs, 1024, base=17000),
        "m": ("LONG", vals, sv_spec(rng, docs, 1 << 14)[2])})


def sumscan_raw_segment(seed, docs):
    """configs[0] with the LONG metric stored raw (no dictionary: Pinot's usual metric layout, noDictionaryColumns):
    8 bytes per doc, read straight from HBM."""
    from pinot_amd.segment import Column
    seg = sumscan_segment(seed, docs)
    m = Column(name="m", data_type="LONG", has_dictionary=False)
    m.raw_values = np.random.default_rng(seed + 5).integers(0, 1 << 29, size=docs, dtype=np.int64)
    seg.columns["m"] = m
    return seg


def star_segment(seed, docs, avg_mv=3):
    from pinot_amd.segment import Column, mv_column_from_flat, segment_from_dict_ids
    rng = np.random.default_rng(seed)
    seg = segment_from_dict_ids("st%d" % seed, docs, {
        "d1": sv_spec(rng, docs, 16), "d2": sv_spec(rng, docs, 32), "d3": sv_spec(rng, docs, 64),
        "d4": sv_spec(rng, docs, 8)})
    lengths = rng.integers(1, 2 * avg_mv, size=docs)
    flat = rng.integers(0, 4096, size=int(lengths.sum())).astype(np.uint32)
    seg.columns["tags"] = mv_column_from_flat("tags", lengths, flat, np.arange(4096, dtype=np.int64) * 11, "INT")
    r = Column(name="r", data_type="DOUBLE", has_dictionary=False)
    r.raw_values = rng.normal(100.0, 30.0, size=docs)
    seg.columns["r"] = r
    return seg


WORKLOADS = {
    # configs[0]: COUNT(*), SUM(m) WHERE day BETWEEN a AND b at ~10 % / ~50 % / 100 % selectivity (day dictionary
    # 17000..17999, uniform)
    "sumscan": (sumscan_segment, [
        ("sel_0p1pct", "SELECT COUNT(*), SUM(m) FROM t WHERE daysSinceEpoch = 17100", 0),
        ("sel_1pct", "SELECT COUNT(*), SUM(m) FROM t WHERE daysSinceEpoch BETWEEN 17100 AND 17109", 0),
        ("count_10pct", "SELECT COUNT(*) FROM t WHERE daysSinceEpoch BETWEEN 17100 AND 17201", 0),
        ("count_100pct", "SELECT COUNT(*) FROM t WHERE daysSinceEpoch BETWEEN 17000 AND 18023", 0),
        ("min_100pct", "SELECT MIN(m) FROM t WHERE daysSinceEpoch BETWEEN 17000 AND 18023", 0),
        ("sel_10pct", "SELECT COUNT(*), SUM(m) FROM t WHERE daysSinceEpoch BETWEEN 17100 AND 17201", 0),
        ("sel_50pct", "SELECT COUNT(*), SUM(m) FROM t WHERE daysSinceEpoch BETWEEN 17100 AND 17611", 0),
        ("sel_100pct", "SELECT COUNT(*), SUM(m) FROM t WHERE daysSinceEpoch BETWEEN 17000 AND 18023", 0),
    ]),
    "sumscan_raw": (sumscan_raw_segment, [
        ("sel_10pct", "SELECT COUNT(*), SUM(m) FROM t WHERE daysSinceEpoch BETWEEN 17100 AND 17201", 0),
        ("sel_50pct", "SELECT COUNT(*), SUM(m) FROM t WHERE daysSinceEpoch BETWEEN 17100 AND 17611", 0),
        ("sel_100pct", "SELECT COUNT(*), SUM(m) FROM t WHERE daysSinceEpoch BETWEEN 17000 AND 18023", 0),
    ]),
    # the north-star shape on configs[0]'s columns: filter + GROUP BY SUM (1024-day key space, raw LONG metric)
    "sumgroup": (sumscan_raw_segment, [
        ("sel_10pct", "SELECT daysSinceEpoch, COUNT(*), SUM(m) FROM t WHERE daysSinceEpoch BETWEEN 17100 AND 17201 "
                      "GROUP BY daysSinceEpoch LIMIT 2000", 0),
        ("sel_50pct", "SELECT daysSinceEpoch, COUNT(*), SUM(m) FROM t WHERE daysSinceEpoch BETWEEN 17100 AND 17611 "
                      "GROUP BY daysSinceEpoch LIMIT 2000", 0),
    ]),
    "sumgroup_dict": (sumscan_segment, [
        ("sel_10pct", "SELECT daysSinceEpoch, COUNT(*), SUM(m) FROM t WHERE daysSinceEpoch BETWEEN 17100 AND 17201 "
                      "GROUP BY daysSinceEpoch LIMIT 2000", 0),
        ("sel_50pct", "SELECT daysSinceEpoch, COUNT(*), SUM(m) FROM t WHERE daysSinceEpoch BETWEEN 17100 AND 17611 "
                      "GROUP BY daysSinceEpoch LIMIT 2000", 0),
    ]),
    # configs[1]: bench.py's AdAnalytics segments and README query (execution statistics: --exec-stats)
    "adanalytics": (lambda seed, docs: _bench().make_segment(seed, docs), [
        ("readme", None, 0),
    ]),
    # configs[1]'s columns with the accountId IN list widened (bench.py's secondary lines): 10 % / 50 % of the docs
    "adanalytics_in": (lambda seed, docs: _bench().make_segment(seed, docs), [
        ("sel_10pct", "@17476", 0),
        ("sel_50pct", "@87381", 0),
    ]),
    "highcard": (highcard_segment, [
        ("all_docs", "SELECT d1, d2, SUM(m), MIN(m), MAX(m) FROM t GROUP BY d1, d2 LIMIT 2000000 "
                     "OPTION(numGroupsLimit=2000000)", 0),
        ("filtered_10pct", "SELECT d1, d2, SUM(m), MIN(m), MAX(m) FROM t WHERE m < 6554 GROUP BY d1, d2 "
                           "LIMIT 2000000 OPTION(numGroupsLimit=2000000)", 0),
        # decomposition of all_docs (which part of the work costs what)
        ("count_only", "SELECT d1, d2, COUNT(*) FROM t GROUP BY d1, d2 LIMIT 2000000 "
                       "OPTION(numGroupsLimit=2000000)", 0),
        ("minmax_only", "SELECT d1, d2, MIN(m), MAX(m) FROM t GROUP BY d1, d2 LIMIT 2000000 "
                        "OPTION(numGroupsLimit=2000000)", 0),
        ("sum_only", "SELECT d1, d2, SUM(m) FROM t GROUP BY d1, d2 LIMIT 2000000 "
                     "OPTION(numGroupsLimit=2000000)", 0),
        # the default numGroupsLimit (100000 < 1M keys): first-seen trimming per segment (a11)
        ("default_limit", "SELECT d1, d2, SUM(m), MIN(m), MAX(m) FROM t GROUP BY d1, d2 LIMIT 2000000", 0),
    ]),
    # configs[2] over segments with their own dictionaries (count-free emit: per-segment key / value id offsets)
    "highcard_own": (highcard_own_segment, [
        ("all_docs", "SELECT d1, d2, SUM(m), MIN(m), MAX(m) FROM t GROUP BY d1, d2 LIMIT 2000000 "
                     "OPTION(numGroupsLimit=2000000)", 0),
        ("filtered_10pct", "SELECT d1, d2, SUM(m), MIN(m), MAX(m) FROM t WHERE m < 6554 GROUP BY d1, d2 "
                           "LIMIT 2000000 OPTION(numGroupsLimit=2000000)", 0),
        ("default_limit", "SELECT d1, d2, SUM(m), MIN(m), MAX(m) FROM t GROUP BY d1, d2 LIMIT 2000000", 0),
    ]),
    "highcard_rd": (highcard_rd_segment, [
        ("all_docs", "SELECT d1, d2, SUM(m), MIN(m), MAX(m) FROM t GROUP BY d1, d2 LIMIT 2000000 "
                     "OPTION(numGroupsLimit=2000000)", 0),
    ]),
    "star": (star_segment, [
        ("all_docs", "SELECT d1, d2, d3, d4, SUM(r), DISTINCTCOUNTHLLMV(tags) FROM t GROUP BY d1, d2, d3, d4 "
                     "LIMIT 1000000 OPTION(numGroupsLimit=1000000)", 0),
        # decomposition of all_docs (which part of the work costs what)
        ("count_only", "SELECT d1, d2, d3, d4, COUNT(*) FROM t GROUP BY d1, d2, d3, d4 "
                       "LIMIT 1000000 OPTION(numGroupsLimit=1000000)", 0),
        ("sum_only", "SELECT d1, d2, d3, d4, SUM(r) FROM t GROUP BY d1, d2, d3, d4 "
                     "LIMIT 1000000 OPTION(numGroupsLimit=1000000)", 0),
        ("hll_only", "SELECT d1, d2, d3, d4, DISTINCTCOUNTHLLMV(tags) FROM t GROUP BY d1, d2, d3, d4 "
                     "LIMIT 1000000 OPTION(numGroupsLimit=1000000)", 0),
        # the default numGroupsLimit (100000 < 262144 keys): first-seen trimming per segment (walk form: SV group-by)
        ("default_limit", "SELECT d1, d2, d3, d4, SUM(r), DISTINCTCOUNTHLLMV(tags) FROM t GROUP BY d1, d2, d3, d4 "
                          "LIMIT 1000000", 0),
    ]),
    # MV group-by (a doc expands into one key per value of tags): 64 x 4096 keys, so the default numGroupsLimit (100000)
    # binds in every segment and the sorted-form first-seen trimming runs (a11'); untrimmed for comparison
    "mvgroup": (star_segment, [
        ("untrimmed", "SELECT d3, tags, COUNT(*), SUM(r) FROM t GROUP BY d3, tags LIMIT 1000000 "
                      "OPTION(numGroupsLimit=1000000)", 0),
        ("default_limit", "SELECT d3, tags, COUNT(*), SUM(r) FROM t GROUP BY d3, tags LIMIT 1000000", 0),
    ]),
}


CHECK_LINES = ("all_docs", "filtered_10pct", "default_limit")


def oracle_check(ex, q, host_segs, sp, rel=0.0):
    """The full-size line's result (every segment of the run) against the oracle's server-level result of the same
    segments, outside the timed region (--check; test infrastructure, as bench.py's oracle_check): keys, counts,
    numDocsScanned, numGroupsLimitReached and every aggregation bit-exact (tests/test_gpu_configs.py _compare_arrays),
    except a SUM over a raw DOUBLE column (rel: the tests' DOUBLE_REL, the atomic order differs from docId order)."""
    import numpy as np
    import oracle
    from pinot_amd import _lib as L
    ex.execute(sp)
    keys, counts, outs = ex.fetch_arrays(sp)
    t0 = time.perf_counter()
    exp = oracle.run_query_arrays(q, host_segs)
    res = {"docs": int(sum(s.num_docs for s in host_segs)), "groups": int(len(exp["keys"])),
           "oracle_s": round(time.perf_counter() - t0, 1)}
    try:
        assert int(L.lib().pa_query_matched_docs(ex.handle)) == exp["matched"], "numDocsScanned"
        assert (int(L.lib().pa_query_num_groups_limit_reached(ex.handle)) > 0) == exp["limit_reached"], "limit"
        np.testing.assert_array_equal(keys, exp["keys"])
        np.testing.assert_array_equal(counts, exp["counts"])
        for a, gi, oi in zip(q.aggregations, ex.agg_map, exp["amap"]):
            if a.function != "COUNT":
                got, want = outs[gi], exp["accs"][oi]
                if rel and a.function == "SUM":
                    np.testing.assert_allclose(got, want, rtol=rel, atol=0, err_msg=a.function)
                    res["sum_max_rel"] = float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))
                else:
                    np.testing.assert_array_equal(got.reshape(want.shape), want, err_msg=a.function)
        res["checked"] = True
    except AssertionError as e:
        res["checked"] = False
        res["error"] = str(e)[:300]
    return res


def cpu_port_baseline(sql, host_segs):
    """bench.py's cpu_baseline (the C oracle port, one segment per thread) over the kept host segments."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("pa_bench_main", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from pinot_amd import parse_sql
    return bench.cpu_baseline(parse_sql(sql), host_segs)


_BENCH = []


def _bench():
    if not _BENCH:
        import importlib.util
        spec = importlib.util.spec_from_file_location("bench_main", os.path.join(ROOT, "bench.py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        _BENCH.append(m)
    return _BENCH[0]


def selection_check(gsegs, host, q, ids, days):
    """selection_topk over the sample of segments kept on the host against a numpy top-K of the same segments: rows in
    (clicks DESC, segment, doc) order, compared as (segment, doc, impressions, clicks)."""
    from pinot_amd.engine import SelectionExecutor
    from pinot_amd.segment import unpack_bits as unpack_all

    def unpack_bits(buf, n, nb, chunk=1 << 20):  # (chunks of whole bytes: the decode's temporaries stay small)
        return np.concatenate([unpack_all(buf[s * nb // 8:], min(chunk, n - s), nb) for s in range(0, n, chunk)])
    ex = SelectionExecutor(q, gsegs[:len(host)])
    got = ex.run()
    ex.close()
    seg_i, doc_i, clicks, imps = [], [], [], []
    for si, sg in enumerate(host):
        val = {n: np.asarray(sg.column(n).dictionary)[unpack_bits(sg.column(n).fwd_bytes, sg.num_docs, sg.column(n).num_bits)]
               for n in ("daysSinceEpoch", "accountId", "clicks", "impressions")}
        m = np.flatnonzero((val["daysSinceEpoch"] >= days[0]) & (val["daysSinceEpoch"] <= days[1]) &
                           np.isin(val["accountId"], ids))
        seg_i.append(np.full(len(m), si))
        doc_i.append(m)
        clicks.append(val["clicks"][m])
        imps.append(val["impressions"][m])
    seg_i, doc_i, clicks, imps = map(np.concatenate, (seg_i, doc_i, clicks, imps))
    top = np.lexsort((doc_i, seg_i, -clicks))[:q.offset + q.limit]
    want = [[int(clicks[i]), int(imps[i])] for i in top]
    ok = (got.segments.tolist() == seg_i[top].tolist() and got.docs.tolist() == doc_i[top].tolist() and
          [[int(r[0]), int(r[1])] for r in got.rows] == want)
    return {"checked": bool(ok), "segments": len(host), "matched": int(len(doc_i))}


def run_selection(nseg, docs, reps, warm=0, check=False, tuning=None, cpu_sample=0):
    """The selection workload: selection_topk and max_same_where, scan ms per launch by HIP events around back-to-back
    launches after `warm` untimed ones. Byte model of selection_topk: bench.algorithmic_bytes of its filter (staged
    columns whole) + the ORDER BY column read per matching doc, sector-wise, + one 64-byte sector per output cell."""
    import torch
    from pinot_amd import parse_sql
    from pinot_amd import _lib as L
    from pinot_amd.engine import GpuQueryExecutor, GpuSegment, SelectionExecutor
    B = _bench()
    keep = max(cpu_sample, 2) if check else 0
    gsegs, cids, host = [], None, []
    for i in range(nseg):
        seg = B.make_segment(100 + i, docs)
        cids = cids or {n: j for j, n in enumerate(sorted(seg.columns))}
        gsegs.append(GpuSegment(seg, column_ids=cids, device=0))
        if len(host) < keep:
            host.append(seg)
            continue
        for c in seg.columns.values():
            c.fwd_bytes = None
    ids = np.sort(np.random.default_rng(4242).choice(B.COLUMNS["accountId"][2](), size=B.SECONDARY[0][1], replace=False))
    sec = B.secondary_query(B.SECONDARY[0][1])
    where = sec[sec.index(" WHERE "):sec.index(" GROUP BY")]
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    lines = (("selection_topk", "SELECT impressions, clicks FROM AdAnalyticsTable%s ORDER BY clicks DESC LIMIT 10" % where),
             ("max_same_where", "SELECT MAX(clicks) FROM AdAnalyticsTable%s" % where))
    for name, sql in lines:
        q = parse_sql(sql)
        ex = (SelectionExecutor if q.is_selection else GpuQueryExecutor)(q, gsegs, tuning=tuning)
        ex.execute(sp)
        for _ in range(warm):
            ex.scan(sp)
        torch.cuda.synchronize()
        ex.reset(sp)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(reps):
            ex.scan(sp)
        b.record(stream)
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / reps
        # reset + scan per launch: a selection's scans above start from the bound the earlier scans published (tighter
        # than a fresh query's all-ones bound), so the figure of a fresh query is this one
        a.record(stream)
        for _ in range(reps):
            ex.execute(sp)
        b.record(stream)
        torch.cuda.synchronize()
        execute_ms = a.elapsed_time(b) / reps
        ex.execute(sp)
        t1 = time.perf_counter()
        res = ex.fetch(sp, execution_stats=False)
        fetch_ms = (time.perf_counter() - t1) * 1e3
        matched = int(L.lib().pa_query_matched_docs(ex.handle))
        algo = B.algorithmic_bytes(ex, matched)
        out = {"workload": "selection", "plan_name": name, "kernel_ms": round(ms, 4),
               "execute_ms": round(execute_ms, 4), "fetch_ms": round(fetch_ms, 2),
               "matched_docs": matched, "plan": ex.stats()["plan"], "segments": nseg, "docs_per_segment": docs,
               "warm": warm, "reps": reps}
        if q.is_selection:
            p = matched / max(1, nseg * docs)
            nb = gsegs[0].segment.column("clicks").num_bits
            algo += int(nseg * docs * nb / 8 * B._touched(p, 512 / nb)) + 64 * len(res.rows) * len(res.columns)
            out.update(rows=len(res.rows), first_row=[int(v) for v in res.rows[0]] if res.rows else None,
                       counters=ex.counters())
            if check:
                out["check"] = selection_check(gsegs, host, q, ids, B.DAY_RANGE)
        else:
            out["max"] = res.row[0]
        out["roofline"] = {"bound": "hbm", "achieved": algo / (ms * 1e-3) / 1e9, "peak": 8000.0, "unit": "GB/s",
                           "frac": algo / (ms * 1e-3) / 1e9 / 8000.0, "algorithmic_bytes_per_launch": algo}
        print(json.dumps(out), flush=True)
        ex.close()
    for g in gsegs:
        g.close()


def run_distinct(nseg, docs, reps, warm=0, tuning=None):
    """The distinct workload: per line the scan ms per launch (HIP events around back-to-back reset + scan launches after
    `warm` untimed ones), the finish (fetch) ms, the strategy, and the algorithmic bytes (the staged bits of the filter
    and DISTINCT columns, bench.algorithmic_bytes) against 8 TB/s; the yardstick lines are GROUP BY COUNT(*) over the
    same columns with the same WHERE."""
    import torch
    from pinot_amd import parse_sql
    from pinot_amd import _lib as L
    from pinot_amd.engine import DistinctExecutor, GpuQueryExecutor, GpuSegment
    B = _bench()
    sec = B.secondary_query(B.SECONDARY[0][1])
    where = sec[sec.index(" WHERE "):sec.index(" GROUP BY")]
    groups = (
        (lambda i: B.make_segment(100 + i, docs), (
            ("a_distinct_days", "SELECT DISTINCT daysSinceEpoch FROM AdAnalyticsTable%s LIMIT 1000" % where, None),
            # the scan taken apart (tuning debug_emit, results invalid: pa_strat_distinct.h "distinct"): without the in-wave
            # combining, without the LDS atomics, without both; and the global variant on the same query
            ("a_distinct_days_no_combine", "SELECT DISTINCT daysSinceEpoch FROM AdAnalyticsTable%s LIMIT 1000" % where,
             {"debug_emit": 4}),
            ("a_distinct_days_no_atomic", "SELECT DISTINCT daysSinceEpoch FROM AdAnalyticsTable%s LIMIT 1000" % where,
             {"debug_emit": 1}),
            ("a_distinct_days_keys_only", "SELECT DISTINCT daysSinceEpoch FROM AdAnalyticsTable%s LIMIT 1000" % where,
             {"debug_emit": 5}),
            ("a_distinct_days_global", "SELECT DISTINCT daysSinceEpoch FROM AdAnalyticsTable%s LIMIT 1000" % where,
             {"distinct_lds": 0}),
            ("a_groupby_count", "SELECT daysSinceEpoch, COUNT(*) FROM AdAnalyticsTable%s GROUP BY daysSinceEpoch "
                                "TOP 1000" % where, None),
            # the same yardstick through the generic kernels the distinct scan shares: STRAT_LDS lane-major, step-major
            ("a_groupby_count_generic", "SELECT daysSinceEpoch, COUNT(*) FROM AdAnalyticsTable%s GROUP BY daysSinceEpoch "
                                        "TOP 1000" % where, "generic"),
            ("a_groupby_count_stepmajor", "SELECT daysSinceEpoch, COUNT(*) FROM AdAnalyticsTable%s GROUP BY "
                                          "daysSinceEpoch TOP 1000" % where, "stepmajor"))),
        (lambda i: highcard_segment(i, docs), (
            ("b_distinct_d1_d2", "SELECT DISTINCT d1, d2 FROM t LIMIT 1000000", None),
            ("b_distinct_d1_d2_global", "SELECT DISTINCT d1, d2 FROM t LIMIT 1000000", {"distinct_lds": 0}),
            ("b_distinct_d1_d2_lds", "SELECT DISTINCT d1, d2 FROM t LIMIT 1000000", {"distinct_lds": 2}),
            # line (b) taken apart: the tile stream alone (PA_QF_DEBUG_STREAM_ONLY), + filter and keys (no word load, no
            # atomic), + the word loads (no atomic), the full scan above; and a plain atomic per doc instead of
            # test-before-set, with and without the in-wave combining
            ("b_stream_only", "SELECT DISTINCT d1, d2 FROM t LIMIT 1000000", "stream"),
            ("b_keys_only", "SELECT DISTINCT d1, d2 FROM t LIMIT 1000000", {"debug_emit": 3}),
            ("b_keys_loads", "SELECT DISTINCT d1, d2 FROM t LIMIT 1000000", {"debug_emit": 1}),
            ("b_plain_atomic", "SELECT DISTINCT d1, d2 FROM t LIMIT 1000000", {"debug_emit": 8}),
            ("b_plain_atomic_no_combine", "SELECT DISTINCT d1, d2 FROM t LIMIT 1000000", {"debug_emit": 12}),
            ("b_no_combine", "SELECT DISTINCT d1, d2 FROM t LIMIT 1000000", {"debug_emit": 4}),
            ("b_groupby_count", "SELECT d1, d2, COUNT(*) FROM t GROUP BY d1, d2 TOP 1000000", None))),
    )
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    for make, lines in groups:
        gsegs, cids = [], None
        for i in range(nseg):
            seg = make(i)
            cids = cids or {n: j for j, n in enumerate(sorted(seg.columns))}
            gsegs.append(GpuSegment(seg, column_ids=cids, device=0))
            for c in seg.columns.values():
                c.fwd_bytes = None
            log("distinct: segment %d of %d resident" % (i + 1, nseg))
        for name, sql, tune in lines:
            q = parse_sql(sql)
            tn = dict(tuning or {}, **(tune if isinstance(tune, dict) else {}))
            flags = 0 if not isinstance(tune, str) else L.PA_QF_DEBUG_STREAM_ONLY if tune == "stream" else (
                L.PA_QF_NO_DENSE_GROUP | L.PA_QF_NO_JIT | (L.PA_QF_NO_LANE_MAJOR if tune == "stepmajor" else 0))
            invalid = tune == "stream" or "debug_emit" in tn  # (a scan that skips work: timed, never fetched)
            ex = (DistinctExecutor(q, gsegs, tuning=tn, force_scan=True, flags=flags) if q.is_distinct
                  else GpuQueryExecutor(q, gsegs, tuning=tn, flags=flags))
            for _ in range(1 + warm):
                ex.execute(sp)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            samples = []
            for _ in range(reps):
                ex.reset(sp)
                a.record(stream)
                ex.scan(sp)
                b.record(stream)
                torch.cuda.synchronize()
                samples.append(a.elapsed_time(b))
            ms = float(np.median(samples))
            out = {"workload": "distinct", "plan_name": name, "kernel_ms": round(ms, 4),
                   "kernel_ms_min": round(min(samples), 4), "kernel_ms_max": round(max(samples), 4),
                   "plan": ex.stats()["plan"], "segments": nseg, "docs_per_segment": docs, "warm": warm, "reps": reps}
            if invalid:
                out["results_invalid"] = tune if isinstance(tune, str) else tn
            else:
                ex.execute(sp)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                res = ex.fetch(sp, execution_stats=False)
                fetch_ms = (time.perf_counter() - t1) * 1e3
                matched = int(L.lib().pa_query_matched_docs(ex.handle))
                algo = B.algorithmic_bytes(ex, matched)
                out.update(fetch_ms=round(fetch_ms, 2), matched_docs=matched,
                           rows=len(res.rows) if q.is_distinct else len(res.groups),
                           roofline={"bound": "hbm", "achieved": algo / (ms * 1e-3) / 1e9, "peak": 8000.0,
                                     "unit": "GB/s", "frac": algo / (ms * 1e-3) / 1e9 / 8000.0,
                                     "algorithmic_bytes_per_launch": algo})
                if q.is_distinct:
                    out["present"] = res.present
            print(json.dumps(out), flush=True)
            ex.close()
        for g in gsegs:
            g.close()


TRIM_SQL = ("SELECT d1, d2, SUM(m), MIN(m), MAX(m) FROM t GROUP BY d1, d2 ORDER BY SUM(m) DESC LIMIT 10 "
            "OPTION(numGroupsLimit=2000000)")


def run_trim(nseg, docs, reps, tuning=None):
    """The group trim line: configs[2] with ORDER BY SUM(m) DESC LIMIT 10 on one executor. (a) host_trim: the full fetch
    (every non-empty group to the host and into Python objects) plus reduce.server_trim — what a server did before the
    device trim, the yardstick; (b) device_trim: fetch(server_trim=True). Per side the device part (HIP events around
    the fetch_arrays call on the launch stream: kernels and copies) and the wall time of the whole call, medians of
    `reps`; the two blocks are compared."""
    import torch
    from pinot_amd import parse_sql
    from pinot_amd import trim as TR
    from pinot_amd.engine import GpuQueryExecutor, GpuSegment
    from pinot_amd.reduce import server_trim
    gsegs = [GpuSegment(highcard_segment(100 + i, docs), device=0) for i in range(nseg)]
    q = parse_sql(TRIM_SQL)
    ex = GpuQueryExecutor(q, gsegs, tuning=tuning)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    ex.execute(sp)
    torch.cuda.synchronize()
    spec = TR.build_spec(TR.lower_order_by(q, ex.agg_map, ex.hashed), TR.trim_size(q))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def device_ms(trim_spec):
        ex.fetch_arrays(sp, pooled=True, trim_spec=trim_spec)  # (warms the allocations)
        out = []
        for _ in range(reps):
            a.record(stream)
            ex.fetch_arrays(sp, pooled=True, trim_spec=trim_spec)
            b.record(stream)
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b))
        return float(np.median(out))

    def wall_ms(fn):
        out, res = [], None
        for _ in range(reps):
            t = time.perf_counter()
            res = fn()
            out.append((time.perf_counter() - t) * 1e3)
        return float(np.median(out)), res

    host_dev = device_ms(None)
    dev_dev = device_ms(spec)
    host_wall, want = wall_ms(lambda: server_trim(ex.fetch(sp, execution_stats=False), q))
    dev_wall, got = wall_ms(lambda: ex.fetch(sp, execution_stats=False, server_trim=True))
    lt = dict(ex.last_trim)
    assert lt["device"] and got.groups == want.groups, lt
    print(json.dumps({"workload": "trim", "plan_name": "order_by_sum_desc_limit10", "sql": TRIM_SQL,
                      "groups": lt["groups"], "kept": lt["kept"],
                      "host_trim": {"device_ms": round(host_dev, 3), "wall_ms": round(host_wall, 2)},
                      "device_trim": {"device_ms": round(dev_dev, 3), "wall_ms": round(dev_wall, 2)},
                      "wall_speedup": round(host_wall / dev_wall, 2), "plan": ex.stats()["plan"],
                      "segments": nseg, "docs_per_segment": docs, "reps": reps}), flush=True)
    ex.close()
    for g in gsegs:
        g.close()


def run(workload, nseg, docs, reps, only=None, no_stepmajor=False, variants=None, cpu_sample=0, exec_stats=False,
        warm=0, check=False, tuning=None):
    import torch
    from pinot_amd import parse_sql
    from pinot_amd import _lib as L
    from pinot_amd.engine import GpuQueryExecutor, GpuSegment
    make, queries = WORKLOADS[workload]
    t0 = time.perf_counter()
    gsegs, cids, host = [], None, []
    for i in range(nseg):
        seg = make(100 + i, docs)
        if cids is None:
            cids = {n: j for j, n in enumerate(sorted(seg.columns))}
        gsegs.append(GpuSegment(seg, column_ids=cids, device=0))
        if check or len(host) < cpu_sample:
            host.append(seg)  # (kept whole for the CPU baseline)
            continue
        for c in seg.columns.values():  # HBM holds the data now; keep only the dictionaries
            c.fwd_bytes = None
            c.raw_values = None
        if (i + 1) % 10 == 0:
            log("  %d/%d segments resident, %.1f s" % (i + 1, nseg, time.perf_counter() - t0))
    log("%s: %d segments x %d docs resident (%.1f GB), %.1f s" % (
        workload, nseg, docs, sum(g.device_bytes for g in gsegs) / 1e9, time.perf_counter() - t0))
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    for name, sql, flags in queries:
        if only and name != only:
            continue
        sql = sql or _bench().QUERY
        if sql.startswith("@"):
            sql = _bench().secondary_query(int(sql[1:]))
        vs = variants or (((0, ""),) if no_stepmajor else ((0, ""), (L.PA_QF_NO_LANE_MAJOR, "_stepmajor")))
        def extra_flags(vs_, tag_):
            return dict((t_, f_) for f_, t_ in vs_)[tag_]
        for extra, tag in vs:
            ex = GpuQueryExecutor(parse_sql(sql), gsegs, tuning=tuning,
                                  flags=flags | extra | (L.PA_QF_NO_FILTER_STATS if exec_stats else 0))
            ex.execute(sp)
            for _ in range(warm):  # (untimed: the clocks reach their steady state)
                ex.scan(sp)
            torch.cuda.synchronize()
            ex.reset(sp)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(reps):
                ex.scan(sp)
            b.record(stream)
            torch.cuda.synchronize()
            ms = a.elapsed_time(b) / reps
            if ex.stats()["plan"]["results_invalid"]:  # (a tuning that skips kernel work: the scan time is all there is)
                print(json.dumps({"workload": workload, "plan_name": name + tag, "kernel_ms": round(ms, 4),
                                  "tuning": tuning, "plan": ex.stats()["plan"], "segments": nseg,
                                  "docs_per_segment": docs}), flush=True)
                ex.close()
                continue
            ex.execute(sp)
            torch.cuda.synchronize()  # fetch_ms = compaction + copies (+ host decode of small blocks) only
            ex.fetch_arrays(sp, pooled=True)  # (first use grows the process's pinned output pool)
            ex.fetch(sp, execution_stats=False)  # (numDocsScanned of this scan)
            t1 = time.perf_counter()
            keys, counts, outs = ex.fetch_arrays(sp, pooled=True)
            fetch_ms = (time.perf_counter() - t1) * 1e3
            # end to end: accumulator reset + scan + fetch of the groups into host arrays, one query after another
            t2 = time.perf_counter()
            for _ in range(3):
                ex.execute(sp)
                ex.fetch_arrays(sp, pooled=True)
            e2e_ms = (time.perf_counter() - t2) * 1e3 / 3
            st = ex.stats()
            extra = {}
            if check and name in CHECK_LINES:
                extra["check"] = oracle_check(ex, parse_sql(sql), host, sp, rel=1e-9 if workload == "star" else 0.0)
                log("%s %s%s: oracle check %s" % (workload, name, tag, extra["check"]))
            # roofline of the fused scan on the byte model every line shares (bench.algorithmic_bytes): staged columns
            # whole, columns read per surviving doc (and multi-value offsets / values) at 64-byte-sector granularity
            matched = int(L.lib().pa_query_matched_docs(ex.handle))
            algo = _bench().algorithmic_bytes(ex, matched)
            extra["roofline"] = {"bound": "hbm", "achieved": algo / (ms * 1e-3) / 1e9, "peak": 8000.0,
                                 "unit": "GB/s", "frac": algo / (ms * 1e-3) / 1e9 / 8000.0,
                                 "algorithmic_bytes_per_launch": algo}
            if cpu_sample:
                extra["cpu_baseline"] = cpu_port_baseline(sql, host)
            if exec_stats:
                # numEntriesScannedInFilter / PostFilter of every segment: (a) an executor whose scan does not count
                # (PA_QF_NO_FILTER_STATS: pa_query_execution_stats' GPU engine over leaf bitmaps); (b) the default
                # executor, whose scan counts a two-leaf AND's leaps itself where that applies: its scan time and the
                # statistics call after it, against the plain scan (ms)
                from pinot_amd import filter_stats as FS
                docs_total = int(L.lib().pa_query_matched_docs(ex.handle))
                ex.execution_stats(sp, docs_total)  # (warms the allocator)
                t3 = time.perf_counter()
                in_f, post = ex.execution_stats(sp, docs_total)
                plain_ms = (time.perf_counter() - t3) * 1e3
                fx = GpuQueryExecutor(parse_sql(sql), gsegs, flags=flags | extra_flags(vs, tag), tuning=tuning)
                fx.execute(sp)
                torch.cuda.synchronize()
                fx.reset(sp)
                a.record(stream)
                for _ in range(reps):
                    fx.scan(sp)
                b.record(stream)
                torch.cuda.synchronize()
                fused_scan_ms = a.elapsed_time(b) / reps
                fx.execute(sp)
                fx.fetch_arrays(sp, pooled=True)  # (numDocsScanned of this scan)
                fdocs = int(L.lib().pa_query_matched_docs(fx.handle))
                fx.execution_stats(sp, fdocs)
                t4 = time.perf_counter()
                f_in, f_post = fx.execution_stats(sp, fdocs)
                fused_host_ms = (time.perf_counter() - t4) * 1e3
                fused = int(L.lib().pa_query_leap_leaf(fx.handle)) >= 0
                fx.close()
                assert (f_in, f_post) == (in_f, post), ((f_in, f_post), (in_f, post))
                extra["exec_stats"] = {"scan_ms": round(ms, 4), "plain_stats_ms": round(plain_ms, 3),
                                       "fused": fused, "fused_scan_ms": round(fused_scan_ms, 4),
                                       "fused_host_ms": round(fused_host_ms, 3),
                                       "overhead_vs_scan": round((fused_scan_ms + fused_host_ms) / ms - 1.0, 4),
                                       "entries_in_filter": in_f, "entries_post_filter": post}
            print(json.dumps(dict({"workload": workload, "plan_name": name + tag, "kernel_ms": round(ms, 4),
                              "rows_per_s": st["num_docs"] / (ms * 1e-3), "staged_bytes": st["staged_bytes"],
                              "staged_GBps": st["staged_bytes"] / (ms * 1e-3) / 1e9, "fetch_ms": round(fetch_ms, 2), "e2e_ms": round(e2e_ms, 2),
                              "groups": int(len(keys)), "matched_docs": int(L.lib().pa_query_matched_docs(ex.handle)),
                              "plan": st["plan"], "segments": nseg, "docs_per_segment": docs}, **extra)), flush=True)
            ex.close()
    for g in gsegs:
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all")
    ap.add_argument("--segments", type=int, default=20)
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=0, help="untimed scans before each line's timed ones")
    ap.add_argument("--check", action="store_true",
                    help="keep every segment on the host and check the full-size results against the oracle")
    ap.add_argument("--plan", default=None, help="only this plan name (e.g. all_docs)")
    ap.add_argument("--no-stepmajor", action="store_true", help="skip the forced step-major variants")
    ap.add_argument("--sweep-part", action="store_true",
                    help="partitioned aggregation: sweep LDS per partition x workgroups per CU")
    ap.add_argument("--flags", type=int, default=None, help="run this one PA_QF_* flag set only")
    ap.add_argument("--exec-stats", action="store_true", help="also time the execution statistics per plan")
    ap.add_argument("--tune", action="append", default=[], metavar="NAME=VALUE",
                    help="a tuning of every query built (pinot_amd/csrc/pa_tuning.h); repeatable")
    ap.add_argument("--cpu-sample", type=int, default=0,
                    help="keep this many segments on the host: roofline + the C-port CPU baseline per line")
    args = ap.parse_args()
    tuning = {n: int(v) for n, v in (t.split("=", 1) for t in args.tune)}
    variants = None if args.flags is None else [(args.flags, "_f%d" % args.flags)]
    if args.sweep_part:
        from pinot_amd import _lib as L
        variants = [(ps << L.PA_QF_PART_SHIFT | wg << L.PA_QF_WG_SHIFT, "_part%d_wg%d" % (ps, wg))
                    for ps in (1, 2, 3) for wg in (0, 1, 2)]
    import torch
    torch.cuda.set_device(0)
    if args.workload == "distinct":
        run_distinct(args.segments, args.docs, args.reps, args.warm, tuning)
        return
    if args.workload == "trim":
        run_trim(args.segments, args.docs, args.reps, tuning)
        return
    if args.workload == "selection":
        run_selection(args.segments, args.docs, args.reps, args.warm, args.check, tuning, args.cpu_sample)
        return
    for w in (WORKLOADS if args.workload == "all" else [args.workload]):
        run(w, args.segments, args.docs, args.reps, args.plan, args.no_stepmajor, variants, args.cpu_sample,
            args.exec_stats, args.warm, args.check, tuning)


if __name__ == "__main__":
    main()
