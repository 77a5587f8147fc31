"""Measures the exact PERCENTILE path: PERCENTILE(clicks, 95), ungrouped and GROUP BY daysSinceEpoch, over bench.py's
AdAnalytics segments (default 16 x 10M docs), next to DISTINCTCOUNT(clicks) over the same segments — the same
accumulator footprint (one cell per (group, value id)), byte stores where the histogram has atomics.

Per query one JSON line: the scan (HIP events around back-to-back scans after a warm-up, as bench.py's kernel time),
and for PERCENTILE the two fetch entry points (host clock around calls that end in a stream synchronise):
pa_query_fetch_histogram through GpuQueryExecutor.fetch (bins -> ValueHistograms) and pa_query_percentiles through
GpuQueryExecutor.percentiles (rank select on the GPU). One process, no profiler. No CPU fallback: without a GPU it fails.

    python tools/bench_percentile.py [--segments 16] [--docs 10000000] [--steps 30] [--warmup 10] [--only NAME]
                                     [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QUERIES = (
    ("percentile_ungrouped", "SELECT PERCENTILE(clicks, 95) FROM AdAnalyticsTable"),
    ("percentile_by_day", "SELECT daysSinceEpoch, PERCENTILE(clicks, 95) FROM AdAnalyticsTable "
                          "GROUP BY daysSinceEpoch LIMIT 1000"),
    ("distinctcount_ungrouped", "SELECT DISTINCTCOUNT(clicks) FROM AdAnalyticsTable"),
    ("distinctcount_by_day", "SELECT daysSinceEpoch, DISTINCTCOUNT(clicks) FROM AdAnalyticsTable "
                             "GROUP BY daysSinceEpoch LIMIT 1000"),
)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=16)
    ap.add_argument("--docs", type=int, default=10_000_000, help="docs per segment")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--flags", type=int, default=0)
    ap.add_argument("--only", default="", help="run only the queries whose name starts with this")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch  # (first: torch's HIP runtime must initialise the device before the library's)
    if not torch.cuda.is_available():
        raise SystemExit("bench_percentile needs a GPU")
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    import bench
    from pinot_amd import parse_sql
    from pinot_amd.engine import GpuQueryExecutor, GpuSegment

    cids, gsegs = None, []
    for i in range(args.segments):
        seg = bench.make_segment(1000 + i, args.docs)
        if cids is None:
            cids = {n: j for j, n in enumerate(sorted(seg.columns))}
        gsegs.append(GpuSegment(seg, columns=("clicks", "daysSinceEpoch"), column_ids=cids, device=0))
        for c in seg.columns.values():
            c.fwd_bytes = None
    stream = torch.cuda.current_stream()
    sptr = stream.cuda_stream
    docs = args.segments * args.docs
    lines = []
    for name, sql in QUERIES:
        if not name.startswith(args.only):
            continue
        q = parse_sql(sql)
        ex = GpuQueryExecutor(q, gsegs, flags=args.flags)
        pct = any(a.function.startswith("PERCENTILE") for a in q.aggregations)
        for _ in range(args.warmup):
            ex.execute(sptr)
        torch.cuda.synchronize()
        ex.reset(sptr)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(args.steps):
            ex.scan(sptr)
        b.record(stream)
        torch.cuda.synchronize()
        scan_ms = a.elapsed_time(b) / args.steps
        ex.execute(sptr)
        torch.cuda.synchronize()

        def host_ms(fn):
            for _ in range(3):
                out = fn()
            t = time.perf_counter()
            for _ in range(args.steps):
                out = fn()
            return (time.perf_counter() - t) / args.steps * 1e3, out

        fetch_ms, res = host_ms(lambda: ex.fetch(sptr, execution_stats=False))
        line = {"query": name, "sql": sql, "segments": args.segments, "docs": docs, "plan": ex.stats()["plan"]["variant"],
                "scan_ms": round(scan_ms, 4), "rows_per_sec": round(docs / (scan_ms * 1e-3), 1),
                "fetch_ms": round(fetch_ms, 4),
                "groups": len(res.groups) if q.group_by else 1}
        if pct:
            sel_ms, (keys, sel) = host_ms(lambda: ex.percentiles(sptr))
            line["percentiles_ms"] = round(sel_ms, 4)
            line["p95_first_group"] = float(sel[len(q.aggregations) - 1][0])
        ex.close()
        lines.append(line)
        print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    for g in gsegs:
        g.close()


if __name__ == "__main__":
    main()
