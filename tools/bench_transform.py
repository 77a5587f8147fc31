"""Measures transform expressions evaluated in the scan against the same query over the materialised raw column (which
also runs without this feature: the baseline), over synthetic segments (default 10 x 10M docs):

    SELECT g, SUM(ADD(a, b)) FROM t [WHERE f = 7] GROUP BY g          against   SELECT g, SUM(e) ... GROUP BY g
    SELECT timeConvert(ts, 'MILLISECONDS', 'DAYS'), COUNT(*) FROM t [WHERE f = 7]
        GROUP BY timeConvert(ts, 'MILLISECONDS', 'DAYS')              against   SELECT d, COUNT(*) ... GROUP BY d

a: dictionary INT (1000 values), b: raw INT, g: dictionary INT (64 values), ts: raw LONG milliseconds over 365 days, f:
dictionary INT (100 values, `f = 7` keeps 1 %); e = (0.0 + a) + b as raw DOUBLE and d = ts / 86400000 as raw LONG are
materialised with transform.evaluate. Both forms run in the same process, alternating, each timed by HIP events around
back-to-back scans after a warm-up (as bench.py's kernel time); the results are compared group by group first. A third
executor runs the materialised query on the step-major scan the expression strategies share (no dense GROUP BY kernel,
no lane-major tiles): what the per-doc walk costs without any expression. The
achieved bytes/s counts the bytes the query needs: the forward-index bits and raw values of every column it reads for
every doc without a filter, and the filter column for every doc plus one 64-byte sector per other column and matching
doc with the 1 % filter. numGroupsLimit is not enforced (the raw day key could bind it on either side). One JSON line
per (query, filter). No profiler, no CPU fallback: without a GPU it fails.

    python tools/bench_transform.py [--segments 10] [--docs 10000000] [--steps 20] [--warmup 5] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCHEMA = {"g": "INT", "f": "INT", "a": "INT", "b": "INT", "ts": "LONG", "e": "DOUBLE", "d": "LONG"}
RAW = ["b", "ts", "e", "d"]
DAY_MS = 86400000


def make_segment(seed, n):
    import numpy as np
    from pinot_amd import parse_sql
    from pinot_amd import transform as T
    from pinot_amd.segment import create_segment
    rng = np.random.default_rng(seed)
    data = {"g": rng.integers(0, 64, n, dtype=np.int32), "f": rng.integers(0, 100, n, dtype=np.int32),
            "a": rng.integers(0, 1000, n, dtype=np.int32), "b": rng.integers(-1000, 1000, n, dtype=np.int32),
            "ts": rng.integers(0, 365 * DAY_MS, n, dtype=np.int64)}
    q = parse_sql("SELECT SUM(ADD(a, b)) FROM t GROUP BY timeConvert(ts, 'MILLISECONDS', 'DAYS')")
    data["e"] = T.evaluate(q.aggregations[0].column, data)
    data["d"] = T.evaluate(q.group_by[0], data)
    return create_segment("seg%d" % seed, data, SCHEMA, no_dictionary_columns=RAW)


def query_bytes(seg, columns, filter_column, selectivity):
    """Bytes one segment's scan needs (module docstring)."""
    def col_bytes(c):
        col = seg.column(c)
        return seg.num_docs * col.num_bits / 8.0 if col.has_dictionary else col.raw_values.nbytes
    if filter_column is None:
        return sum(col_bytes(c) for c in columns)
    return col_bytes(filter_column) + 64.0 * selectivity * seg.num_docs * len(columns)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=10)
    ap.add_argument("--docs", type=int, default=10_000_000, help="docs per segment")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the expression scan and the baseline scan")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch  # (first: torch's HIP runtime must initialise the device before the library's)
    if not torch.cuda.is_available():
        raise SystemExit("bench_transform needs a GPU")
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    from pinot_amd import _lib as L
    from pinot_amd import parse_sql
    from pinot_amd.engine import GpuQueryExecutor, GpuSegment

    # one generated segment, resident `segments` times (each copy its own device memory)
    seg = make_segment(1, args.docs)
    cids = {n: j for j, n in enumerate(sorted(seg.columns))}
    gsegs = [GpuSegment(seg, column_ids=cids, device=0) for _ in range(args.segments)]
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

    shapes = [
        ("sum_add", "SELECT g, SUM(ADD(a, b)) FROM t%s GROUP BY g LIMIT 1000", "SELECT g, SUM(e) FROM t%s GROUP BY g LIMIT 1000",
         ["g", "a", "b"], ["g", "e"]),
        ("group_by_day", "SELECT timeConvert(ts, 'MILLISECONDS', 'DAYS'), COUNT(*) FROM t%s GROUP BY "
         "timeConvert(ts, 'MILLISECONDS', 'DAYS') LIMIT 1000", "SELECT d, COUNT(*) FROM t%s GROUP BY d LIMIT 1000", ["ts"], ["d"]),
    ]
    lines = []
    for name, expr_sql, mat_sql, expr_cols, mat_cols in shapes:
        for fname, where, fcol, sel in (("dense", "", None, 1.0), ("one_percent", " WHERE f = 7", "f", 0.01)):
            ex_e = GpuQueryExecutor(parse_sql(expr_sql % where), gsegs, enforce_num_groups_limit=False)
            ex_m = GpuQueryExecutor(parse_sql(mat_sql % where), gsegs, enforce_num_groups_limit=False)
            ex_s = GpuQueryExecutor(parse_sql(mat_sql % where), gsegs, enforce_num_groups_limit=False,
                                    flags=L.PA_QF_NO_DENSE_GROUP | L.PA_QF_NO_LANE_MAJOR)
            for ex in (ex_e, ex_m, ex_s):
                for _ in range(args.warmup):
                    ex.execute(sptr)
            torch.cuda.synchronize()
            # equal work first: the expression query's groups against the materialised query's
            re_, rm = ex_e.fetch(sptr, execution_stats=False), ex_m.fetch(sptr, execution_stats=False)
            assert len(re_.groups) == len(rm.groups) and re_.num_docs_scanned == rm.num_docs_scanned
            for key, row in rm.groups.items():
                assert re_.groups[key] == row, (name, fname, key, re_.groups[key], row)
            t_e, t_m, t_s = [], [], []
            for _ in range(args.rounds):
                t_e.append(timed(ex_e))
                t_m.append(timed(ex_m))
                t_s.append(timed(ex_s))
            be, bm = min(t_e), min(t_m)
            bytes_e = args.segments * query_bytes(seg, expr_cols, fcol, sel)
            bytes_m = args.segments * query_bytes(seg, mat_cols, fcol, sel)
            line = {"shape": name, "filter": fname, "segments": args.segments, "docs": docs,
                    "expr_plan": ex_e.stats()["plan"]["variant"], "expr_steps": ex_e.stats()["plan"]["steps"],
                    "materialised_plan": ex_m.stats()["plan"]["variant"],
                    "expr_scan_ms": round(be, 4), "expr_scan_ms_rounds": [round(v, 4) for v in t_e],
                    "materialised_scan_ms": round(bm, 4), "materialised_scan_ms_rounds": [round(v, 4) for v in t_m],
                    "expr_over_materialised": round(be / bm, 4),
                    "materialised_step_major_plan": ex_s.stats()["plan"]["variant"],
                    "materialised_step_major_lane_major": ex_s.stats()["plan"]["lane_major"],
                    "materialised_step_major_scan_ms": round(min(t_s), 4),
                    "expr_bytes": int(bytes_e), "materialised_bytes": int(bytes_m),
                    "expr_gbytes_per_s": round(bytes_e / be / 1e6, 1), "materialised_gbytes_per_s": round(bytes_m / bm / 1e6, 1),
                    "num_docs_scanned": re_.num_docs_scanned, "groups": len(re_.groups)}
            lines.append(line)
            print(json.dumps(line), flush=True)
            for ex in (ex_e, ex_m, ex_s):
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
