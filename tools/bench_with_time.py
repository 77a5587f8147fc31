"""Measures LASTWITHTIME against MAX of its time column, over synthetic segments (default 4 x 4M docs, 1000 groups):

    SELECT g, MAX(ts) FROM t GROUP BY g                       the yardstick, on the plan the planner picks for it: the packed
                                                               form does the same work per matching doc (one column decode,
                                                               one 64-bit max after the wave pre-reduction)
    SELECT g, LASTWITHTIME(v, ts, 'LONG') FROM t GROUP BY g   packed form (one scan launch)
    the same with tuning time_rows_wide = 1                   wide form (two scan launches)
    SELECT g, MAX(ts) ... on the step-major LDS scan          (PA_QF_NO_DENSE_GROUP | PA_QF_NO_LANE_MAJOR: the walk the
                                                               row-by-time strategies share, without the new update)

g: dictionary INT (1000 values), v: dictionary LONG, ts: raw LONG (distinct values per segment). The executors run in
one process, alternating, each timed by HIP events around back-to-back scans after a warm-up (as bench.py's kernel time:
the accumulators are reset once, the scans' results are idempotent maxima); the two forms' fetched rows are compared
first, and the packed form's times with MAX(ts). One JSON line. No profiler, no CPU fallback: without a GPU it fails.

    python tools/bench_with_time.py [--segments 4] [--docs 4000000] [--groups 1000] [--steps 20] [--warmup 5] [--rounds 3]
                                    [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCHEMA = {"g": "INT", "v": "LONG", "ts": "LONG"}


def make_segment(seed, n, groups):
    import numpy as np
    from pinot_amd.segment import create_segment
    rng = np.random.default_rng(seed)
    data = {"g": rng.integers(0, groups, n, dtype=np.int32), "v": rng.integers(0, 5000, n, dtype=np.int64) * 7,
            "ts": rng.permutation(n).astype(np.int64) + 1_600_000_000_000}
    return create_segment("seg%d" % seed, data, SCHEMA, no_dictionary_columns=["ts"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=4)
    ap.add_argument("--docs", type=int, default=4_000_000, help="docs per segment")
    ap.add_argument("--groups", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the executors")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    args = ap.parse_args()

    import torch  # (first: torch's HIP runtime must initialise the device before the library's)
    if not torch.cuda.is_available():
        raise SystemExit("bench_with_time needs a GPU")
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    from pinot_amd import _lib as L
    from pinot_amd import parse_sql
    from pinot_amd.engine import GpuQueryExecutor, GpuSegment

    # one generated segment, resident `segments` times (each copy its own device memory)
    seg = make_segment(1, args.docs, args.groups)
    cids = {n: j for j, n in enumerate(sorted(seg.columns))}
    gsegs = [GpuSegment(seg, column_ids=cids, device=0) for _ in range(args.segments)]
    stream = torch.cuda.current_stream()
    sptr = stream.cuda_stream

    def timed(ex):
        ex.reset(sptr)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(args.steps):
            ex.scan(sptr)
        b.record(stream)
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.steps

    mx = "SELECT g, MAX(ts) FROM t GROUP BY g LIMIT 100000"
    lw = "SELECT g, LASTWITHTIME(v, ts, 'LONG') FROM t GROUP BY g LIMIT 100000"
    exs = {
        "max_ts": GpuQueryExecutor(parse_sql(mx), gsegs),
        "max_ts_step_major_lds": GpuQueryExecutor(parse_sql(mx), gsegs, flags=L.PA_QF_NO_DENSE_GROUP | L.PA_QF_NO_LANE_MAJOR),
        "last_packed": GpuQueryExecutor(parse_sql(lw), gsegs),
        "last_wide": GpuQueryExecutor(parse_sql(lw), gsegs, tuning={"time_rows_wide": 1}),
    }
    for ex in exs.values():
        for _ in range(args.warmup):
            ex.execute(sptr)
    torch.cuda.synchronize()
    res = {k: ex.fetch(sptr, execution_stats=False) for k, ex in exs.items()}
    assert res["last_packed"].groups == res["last_wide"].groups and len(res["last_packed"].groups) == len(res["max_ts"].groups)
    for key, row in res["max_ts"].groups.items():
        assert res["last_packed"].groups[key][0].time == int(row[0]), (key, res["last_packed"].groups[key], row)
    assert exs["last_packed"].stats()["plan"]["time_row_form"] == {0: 1}
    assert exs["last_wide"].stats()["plan"]["time_row_form"] == {0: 2}
    times = {k: [] for k in exs}
    for _ in range(args.rounds):
        for k, ex in exs.items():
            times[k].append(timed(ex))
    line = {"segments": args.segments, "docs": args.segments * args.docs, "groups": len(res["max_ts"].groups),
            "steps": args.steps, "warmup": args.warmup}
    for k, ex in exs.items():
        line[k + "_plan"] = ex.stats()["plan"]["variant"]
        line[k + "_scan_ms"] = round(min(times[k]), 4)
        line[k + "_scan_ms_rounds"] = [round(v, 4) for v in times[k]]
    line["packed_over_max_ts"] = round(line["last_packed_scan_ms"] / line["max_ts_scan_ms"], 3)
    line["wide_over_packed"] = round(line["last_wide_scan_ms"] / line["last_packed_scan_ms"], 3)
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    for ex in exs.values():
        ex.close()
    for g in gsegs:
        g.close()


if __name__ == "__main__":
    main()
