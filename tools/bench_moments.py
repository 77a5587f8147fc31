"""Measures VAR_POP on the moments scan against the hand-written power sums it replaces, over synthetic segments in
configs[1]'s shape (default 4 x 4M docs; d: dictionary INT, 512 values, 9 bits; mi: dictionary LONG, 2^14 values inside
int32, 14 bits; md: dictionary DOUBLE, 2^14 values, 14 bits):

    SELECT d, VAR_POP(m) FROM t GROUP BY d                     m = mi: integer form, m = md: double form; each on the
                                                               planner's variant (LDS) and with PA_QF_FORCE_GLOBAL
    SELECT d, COUNT(*), SUM(m), SUM(m * m) FROM t GROUP BY d   the yardstick: the expression strategy (STRAT_EXPR*), whose
                                                               kernels this change leaves byte-identical
                                                               (profiles/kernel_resources.csv)

The executors run in one process, alternating, each timed by HIP events around back-to-back scans after a warm-up (as
bench.py's kernel time; the accumulators are reset once per window — sums keep growing, which changes no timing); the
variance from the moments and from the power sums are compared first. One JSON line: per executor the minimum and
every round, the yardstick's own spread (max / min - 1 over its rounds), the bytes the query needs (the forward-index
bits of d and m) and that over time as a fraction of 8 TB/s — a whole-scan rate over needed bytes, not a kernel's share
of peak. No profiler, no CPU fallback: without a GPU it fails.

    python tools/bench_moments.py [--segments 4] [--docs 4000000] [--steps 20] [--warmup 5] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12


def make_segment(seed, docs):
    import numpy as np
    from pinot_amd.segment import segment_from_dict_ids
    rng = np.random.default_rng(seed)
    dicts = {"d": ("INT", np.arange(17532, 17532 + 512, dtype=np.int64)),
             "mi": ("LONG", np.arange(1 << 14, dtype=np.int64) * 3),
             "md": ("DOUBLE", 1e6 + np.arange(1 << 14, dtype=np.float64) * 0.37)}
    specs = {}
    for name, (dt, d) in dicts.items():
        nb = int(len(d) - 1).bit_length()  # (every cardinality a power of two: uniform dictIds = random bytes)
        specs[name] = (dt, d, np.frombuffer(rng.bytes((docs * nb + 7) // 8), dtype=np.uint8))
    return segment_from_dict_ids("moments_%d" % seed, docs, specs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=4)
    ap.add_argument("--docs", type=int, default=4_000_000, help="docs per segment")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the executors")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    args = ap.parse_args()

    import torch  # (first: torch's HIP runtime must initialise the device before the library's)
    if not torch.cuda.is_available():
        raise SystemExit("bench_moments needs a GPU")
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    from pinot_amd import _lib as L
    from pinot_amd import parse_sql
    from pinot_amd import reduce as R
    from pinot_amd.engine import GpuQueryExecutor, GpuSegment

    seg = make_segment(1, args.docs)
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

    var = "SELECT d, VAR_POP(%s) FROM t GROUP BY d LIMIT 100000"
    pws = "SELECT d, COUNT(*), SUM(%s), SUM(%s * %s) FROM t GROUP BY d LIMIT 100000"
    exs = {}
    for tag, m in (("int", "mi"), ("double", "md")):
        exs["power_sums_" + tag] = GpuQueryExecutor(parse_sql(pws % (m, m, m)), gsegs)
        exs["var_pop_" + tag] = GpuQueryExecutor(parse_sql(var % m), gsegs)
        exs["var_pop_%s_global" % tag] = GpuQueryExecutor(parse_sql(var % m), gsegs, flags=L.PA_QF_FORCE_GLOBAL)
    for ex in exs.values():
        for _ in range(args.warmup):
            ex.execute(sptr)
    torch.cuda.synchronize()
    res = {k: ex.fetch(sptr, execution_stats=False) for k, ex in exs.items()}
    for tag in ("int", "double"):
        for key, (n, s1, s2) in res["power_sums_" + tag].groups.items():
            want = s2 / n - (s1 / n) ** 2
            for name in ("var_pop_" + tag, "var_pop_%s_global" % tag):
                got = R.final_value("VARPOP", res[name].groups[key][0])
                assert abs(got - want) <= 1e-5 * abs(want), (name, key, got, want)
    times = {k: [] for k in exs}
    for _ in range(args.rounds):
        for k, ex in exs.items():
            times[k].append(timed(ex))
    docs = args.segments * args.docs
    need = docs * (9 + 14) / 8.0
    line = {"segments": args.segments, "docs": docs, "groups": len(res["var_pop_int"].groups), "steps": args.steps,
            "warmup": args.warmup, "rounds": args.rounds, "needed_bytes": int(need)}
    for k, ex in exs.items():
        plan = ex.stats()["plan"]
        line[k + "_plan"] = plan["variant"]
        line[k + "_scan_ms"] = round(min(times[k]), 4)
        line[k + "_scan_ms_rounds"] = [round(v, 4) for v in times[k]]
        line[k + "_fraction_of_8TBps"] = round(need / (min(times[k]) * 1e-3) / HBM_BYTES_PER_S, 4)
        if plan["moments_form"]:
            line[k + "_form"] = list(plan["moments_form"].values())[0]
    for tag in ("int", "double"):
        base = times["power_sums_" + tag]
        line["power_sums_%s_spread" % tag] = round(max(base) / min(base) - 1, 4)
        line["var_pop_%s_over_power_sums" % tag] = round(min(times["var_pop_" + tag]) / min(base), 3)
        line["var_pop_%s_global_over_power_sums" % tag] = round(min(times["var_pop_%s_global" % tag]) / min(base), 3)
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
