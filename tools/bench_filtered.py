"""Measures filtered aggregations against the one-query-per-lane plan, over bench.py's AdAnalytics segments (default
16 x 10M docs):

    SELECT daysSinceEpoch, SUM(clicks) FILTER (WHERE accountId IN <list A>), SUM(clicks) FILTER (WHERE accountId IN
    <list B>), COUNT(*) FROM AdAnalyticsTable [WHERE daysSinceEpoch BETWEEN lo AND hi] GROUP BY daysSinceEpoch

as ONE fused scan (the lanes' masks over the docs the WHERE kept, the columns streamed once), and as the baseline the
engine had before FILTER clauses: one unfiltered query per lane with the lane's filter moved into WHERE (`W AND F_j`,
and W alone for COUNT(*)), which run kernels the filtered path does not touch. Both run in the same process,
alternating, each timed by HIP events around back-to-back scans after a warm-up (as bench.py's kernel time). One JSON
line per shape: the fused scan's time, each baseline scan's time and their sum. No profiler, no CPU fallback: without a
GPU it fails.

    python tools/bench_filtered.py [--segments 16] [--docs 10000000] [--steps 30] [--warmup 10] [--rounds 3]
                                   [--out FILE]
"""
import argparse
import dataclasses
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=16)
    ap.add_argument("--docs", type=int, default=10_000_000, help="docs per segment")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the fused scan and the baseline scans")
    ap.add_argument("--list", type=int, default=40, help="accountIds per IN list")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch  # (first: torch's HIP runtime must initialise the device before the library's)
    if not torch.cuda.is_available():
        raise SystemExit("bench_filtered needs a GPU")
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    import numpy as np
    import bench
    from pinot_amd import parse_sql
    from pinot_amd import query as Q
    from pinot_amd.engine import GpuQueryExecutor, GpuSegment

    cids, gsegs, accounts, days = None, [], None, None
    for i in range(args.segments):
        seg = bench.make_segment(1000 + i, args.docs)
        if cids is None:
            cids = {n: j for j, n in enumerate(sorted(seg.columns))}
            accounts = np.asarray(seg.column("accountId").dictionary)
            days = np.asarray(seg.column("daysSinceEpoch").dictionary)
        gsegs.append(GpuSegment(seg, columns=("clicks", "daysSinceEpoch", "accountId"), column_ids=cids, device=0))
        for c in seg.columns.values():
            c.fwd_bytes = None
    pick = np.linspace(0, len(accounts) - 1, 2 * args.list).astype(int)
    list_a = ", ".join(str(v) for v in accounts[pick[0::2]].tolist())
    list_b = ", ".join(str(v) for v in accounts[pick[1::2]].tolist())
    lo, hi = int(days[len(days) // 4]), int(days[(3 * len(days)) // 4])
    stream = torch.cuda.current_stream()
    sptr = stream.cuda_stream
    docs = args.segments * args.docs

    def timed(ex):
        ex.reset(sptr)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(args.steps):
            ex.scan(sptr)
        b.record(stream)
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.steps

    lines = []
    for name, where in (("no_where", ""), ("day_range", " WHERE daysSinceEpoch BETWEEN %d AND %d" % (lo, hi))):
        sql = ("SELECT daysSinceEpoch, SUM(clicks) FILTER (WHERE accountId IN (%s)), SUM(clicks) FILTER (WHERE accountId "
               "IN (%s)), COUNT(*) FROM AdAnalyticsTable%s GROUP BY daysSinceEpoch LIMIT 1000" % (list_a, list_b, where))
        q = parse_sql(sql)
        fused = GpuQueryExecutor(q, gsegs)
        lanes = []
        for f in (q.aggregations[0].filter, q.aggregations[1].filter, None):
            aggs = [dataclasses.replace(a, filter=None) for a in q.aggregations if a.filter == f]
            filt = q.filter if f is None else (f if q.filter is None else Q.And((q.filter, f)))
            lq = dataclasses.replace(q, aggregations=aggs, aliases=[None] * len(aggs), filter=filt,
                                     num_select_aggs=len(aggs))
            lanes.append(GpuQueryExecutor(lq, gsegs))
        for ex in [fused] + lanes:
            for _ in range(args.warmup):
                ex.execute(sptr)
        torch.cuda.synchronize()
        fused_ms, lane_ms = [], [[] for _ in lanes]
        for _ in range(args.rounds):
            fused_ms.append(timed(fused))
            for k, ex in enumerate(lanes):
                lane_ms[k].append(timed(ex))
        # the fused result against the baseline's, group by group (the measurement compares equal work)
        fused.execute(sptr)
        res = fused.fetch(sptr)
        for k, ex in enumerate(lanes):
            ex.execute(sptr)
            lr = ex.fetch(sptr, execution_stats=False)
            for key, row in lr.groups.items():
                assert res.groups[key][k] == row[0], (name, k, key, res.groups[key], row)
        best = lambda v: min(v)
        line = {"shape": name, "sql_where": where.strip(), "segments": args.segments, "docs": docs, "lanes": 3,
                "in_list": args.list, "fused_plan": fused.stats()["plan"]["variant"],
                "fused_steps": fused.stats()["plan"]["steps"],
                "lane_plans": [ex.stats()["plan"]["variant"] for ex in lanes],
                "fused_scan_ms": round(best(fused_ms), 4), "fused_scan_ms_rounds": [round(v, 4) for v in fused_ms],
                "lane_scan_ms": [round(best(v), 4) for v in lane_ms],
                "lanes_sum_ms": round(sum(best(v) for v in lane_ms), 4),
                "fused_staged_bytes": fused.stats()["staged_bytes"],
                "lanes_staged_bytes": [ex.stats()["staged_bytes"] for ex in lanes],
                "num_docs_scanned": res.num_docs_scanned, "groups": len(res.groups)}
        line["fused_over_lanes"] = round(line["fused_scan_ms"] / line["lanes_sum_ms"], 4)
        lines.append(line)
        print(json.dumps(line), flush=True)
        for ex in [fused] + lanes:
            ex.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    for g in gsegs:
        g.close()


if __name__ == "__main__":
    main()
