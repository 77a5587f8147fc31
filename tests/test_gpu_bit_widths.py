"""Every forward-index decoder at every bit width: the (path, width) matrix.

The forward-index width nb (1..31) selects the code that runs in each decoder (decode_lds / decode_global / decode_batch,
leaf_lm<nb>, lane_agg_lm<NB>, gd_* / gdl_top<NB> / gdl_idv<NB>, the hiprtc kernels' unpack<C, TOP>, stage_tile's partial
DMA instruction). Each case builds (or takes from the module's cache) the two-segment table of width_tables.py whose
column in the path's role (group key g, second key h, aggregated value v, filter f) is nb bits wide, creates the executor
with the flags that force the path, asserts from stats()["plan"] (and pa_query_column_staged) that the path was taken,
and compares the result bit-exactly with width_tables.reference: numpy over the generated ids and dictionaries.

References by kind of path (RUNNERS): numpy for aggregations and GROUP BY (direct and hashed key spaces); the oracle for
numGroupsLimit, the MV paths and DISTINCTCOUNTHLLMV (tests/test_bit_widths_oracle.py pins the oracle against numpy at
every width first, MV stream included); the numpy restatements filtered_ref.numpy_eval, selection_ref.run and
distinct_ref.completed_server, transform_ref.reference for expressions; numpy bitmaps for pa_query_leaf_bitmaps and
numpy counts for pa_query_filter_counts.

Widths: every path runs at every nb in 1..31 in the sweep regime of its role (padded over the natural cardinality from
the natural width up, cardinality 2^nb below it), and again in the full regime (a real dictionary of 2^nb values, ids
with every bit set) at every nb above the role's natural width up to the path's `full_max`: a (path, nb) case runs
both where both exist. A (path, width) pair is left out only through EXCLUDED below.
"""
import ctypes
from dataclasses import dataclass, field

import numpy as np
import pytest

import width_tables as W
from pinot_amd import _lib as L
from pinot_amd import parse_sql
from pinot_amd.engine import GpuQueryExecutor, GpuSegment

pytestmark = pytest.mark.gpu

GRID = {"scan_grid": 2}  # two workgroups: every wave owns several tiles of a segment (the hoisted steady-state loops)
AGG4 = (("COUNT", None), ("SUM", "v"), ("MIN", "v"), ("MAX", "v"))
CNT_SUM = (("COUNT", None), ("SUM", "v"))
MIXED = (("SUM", "v"), ("MIN", "v"), ("MAX", "v"), ("SUM", "ri"))  # (kLaneAggs = 4 aggregations at most)
DENSE, SPARSE, RARE = 0.9, 0.1, 0.0005  # fraction of f's dictIds the filter keeps (RARE: one id, the planted docs' 0)

# full-regime bounds: a value / filter dictionary of 2^20 entries (8 MiB) is cheap. A group key of 2^nb values makes a
# table-wide key space of 2 * 2^nb keys (two dictionaries) times the other key's: the LDS strategy holds accumulator
# blocks up to 64 KiB (pa_plan_kernels.hip plan_strategy: P.lds_acc <= 64 * 1024), i.e. 2048 keys of COUNT + 3 slots:
# g up to 6 bits next to h's 10 keys, h up to 4 bits next to g's 48 keys; the global paths take wider keys
FULL_V, FULL_G, FULL_H, FULL_G_GLOBAL = 20, 6, 4, 12


@dataclass(frozen=True)
class Path:
    role: str                    # the column nb bits wide
    aggs: tuple
    group_by: tuple = ()
    frac: float = DENSE          # None: no filter
    flags: int = 0
    vtype: str = "LONG"
    shared: bool = False
    full_max: int = 0            # the full regime runs at natural width < nb <= full_max
    plan: dict = field(default_factory=dict, hash=False, compare=False)     # plan field -> value | tuple | callable
    staged: dict = field(default_factory=dict, hash=False, compare=False)   # column -> pa_query_column_staged
    kind: str = "numpy"          # the runner and reference: RUNNERS below
    sql: str = ""                # other kinds: the query, {lo} / {hi} = the filter's bounds on f, {m..} see _mv_literals
    tuning: dict = field(default_factory=dict, hash=False, compare=False)
    attrs: dict = field(default_factory=dict, hash=False, compare=False)    # executor attribute -> value


def _lm(v):
    return v.startswith("gdense_lm")


def _agg(role_paths):
    """Aggregation-only paths: the value column v at nb (and the filter column under two of them)."""
    P = {}
    lane = {"strategy": "lane", "variant": "lane_dict", "lane_major": 1}
    for vt in ("LONG", "INT", "DOUBLE"):   # LM_SUM_LONG / LM_SUM_INT / LM_SUM_DOUBLE, MIN / MAX on sorted dictIds
        P["lane_lm_dense_%s" % vt.lower()] = Path("v", AGG4, frac=DENSE, vtype=vt, full_max=FULL_V, plan=lane,
                                                  staged={"v": 1})
    P["lane_lm_sparse"] = Path("v", AGG4, frac=SPARSE, full_max=FULL_V, plan=lane, staged={"v": 1})
    P["lane_lm_lazy"] = Path("v", AGG4, frac=RARE, full_max=FULL_V, plan=lane, staged={"v": 0})
    P["lane_lm_stage_all"] = Path("v", AGG4, frac=RARE, flags=L.PA_QF_STAGE_ALL, full_max=FULL_V, plan=lane,
                                  staged={"v": 1})
    # a dictionary both segments share: SUM through the LDS histogram of dictIds (up to kLaneHistMax = 16384 ids), and
    # the per-doc gather of the same table
    P["lane_lm_shared_hist"] = Path("v", AGG4, frac=DENSE, shared=True, full_max=14, plan=lane, staged={"v": 1})
    P["lane_lm_shared_no_hist"] = Path("v", AGG4, frac=DENSE, shared=True, flags=L.PA_QF_NO_LANE_HIST, full_max=14,
                                       plan=lane, staged={"v": 1})
    # aggregations over a raw and a dictionary column: the mixed kernel (STRAT_LANE), whose lane-major tiles unpack the
    # lane's 32 dictIds statically (lane_agg_lm<NB> through lane_agg_lm_any) when a lane holds more than 12 matching docs
    # and decode per matching doc below that
    mixed = {"strategy": "lane", "variant": "lane", "lane_major": 1}
    for vt in ("LONG", "INT", "DOUBLE"):
        P["lane_lm_mixed_dense_%s" % vt.lower()] = Path("v", MIXED, frac=DENSE, vtype=vt, full_max=FULL_V, plan=mixed,
                                                        staged={"v": 1})
    P["lane_lm_mixed_all_docs"] = Path("v", MIXED, frac=1.0, full_max=FULL_V, plan=mixed, staged={"v": 1})
    P["lane_lm_mixed_sparse"] = Path("v", MIXED, frac=SPARSE, full_max=FULL_V, plan=mixed, staged={"v": 1})
    P["lane_lm_mixed_lazy"] = Path("v", MIXED, frac=RARE, full_max=FULL_V, plan=mixed, staged={"v": 0})
    sm = {"strategy": "lane", "variant": "lane", "lane_major": 0}
    P["lane_sm_dense"] = Path("v", AGG4, frac=DENSE, flags=L.PA_QF_NO_LANE_MAJOR, full_max=FULL_V, plan=sm,
                              staged={"v": 1})
    P["lane_sm_lazy"] = Path("v", AGG4, frac=RARE, flags=L.PA_QF_NO_LANE_MAJOR, full_max=FULL_V, plan=sm,
                             staged={"v": 0})
    P["lane_sm_stage_all"] = Path("v", AGG4, frac=RARE, flags=L.PA_QF_NO_LANE_MAJOR | L.PA_QF_STAGE_ALL,
                                  full_max=FULL_V, plan=sm, staged={"v": 1})
    # the filter column at nb under the lane accumulators (leaf_lm<nb> / the step-major leaf in scan_kernel)
    P["lane_lm_dense_f"] = Path("f", AGG4, frac=DENSE, full_max=FULL_V, plan=lane)
    P["lane_sm_dense_f"] = Path("f", AGG4, frac=DENSE, flags=L.PA_QF_NO_LANE_MAJOR, full_max=FULL_V, plan=sm)
    # LDS and global accumulators, both layouts
    na = L.PA_QF_NO_LANE_ACC
    P["agg_lds_lm"] = Path("v", AGG4, flags=na, full_max=FULL_V, plan={"strategy": "lds", "lane_major": 1})
    P["agg_lds_sm"] = Path("v", AGG4, flags=na | L.PA_QF_NO_LANE_MAJOR, full_max=FULL_V,
                           plan={"strategy": "lds", "lane_major": 0})
    P["agg_global_lm"] = Path("v", AGG4, frac=RARE, flags=na | L.PA_QF_FORCE_GLOBAL, full_max=FULL_V,
                              plan={"strategy": "global", "lane_major": 1})
    P["agg_global_sm"] = Path("v", AGG4, flags=na | L.PA_QF_FORCE_GLOBAL | L.PA_QF_NO_LANE_MAJOR, full_max=FULL_V,
                              plan={"strategy": "global", "lane_major": 0})
    role_paths.update(P)


def _group_by(role_paths):
    """GROUP BY on LDS / global accumulators: the key g, the second key h, the value v and the filter f at nb in turn."""
    nd = L.PA_QF_NO_DENSE_GROUP
    for role in ("g", "h", "v", "f"):
        fm = FULL_V if role in "vf" else (FULL_G if role == "g" else FULL_H)
        fmg = FULL_V if role in "vf" else (FULL_G_GLOBAL if role == "g" else 8)
        gb = ("g", "h")
        lds_lm = {"strategy": "lds", "lane_major": 1}
        lds_sm = {"strategy": "lds", "lane_major": 0}
        P = {}
        # accumulate_lds_lm: KB 4 (a tile of up to 512 matches) and KB 8 (more)
        P["gb_lds_lm_kb4"] = Path(role, AGG4, gb, SPARSE, nd, full_max=fm, plan=lds_lm)
        P["gb_lds_lm_kb8"] = Path(role, AGG4, gb, DENSE, nd, full_max=fm, plan=lds_lm)
        P["gb_lds_lazy_post"] = Path(role, AGG4, gb, DENSE, L.PA_QF_LAZY_POST, full_max=fm, plan=lds_lm,
                                     staged={"g": 0, "h": 0, "v": 0})
        # accumulate_step; 16- and 32-step tiles (the partial DMA instruction differs)
        P["gb_lds_sm"] = Path(role, AGG4, gb, DENSE, L.PA_QF_NO_LANE_MAJOR, full_max=fm, plan=lds_sm)
        P["gb_lds_steps16"] = Path(role, AGG4, gb, DENSE, L.PA_QF_STEPS16, full_max=fm, plan=dict(lds_sm, steps=16))
        P["gb_lds_steps32"] = Path(role, AGG4, gb, DENSE, L.PA_QF_STEPS32 | L.PA_QF_NO_LANE_MAJOR, full_max=fm,
                                   plan=dict(lds_sm, steps=32))
        P["gb_global_lm"] = Path(role, AGG4, gb, RARE, L.PA_QF_FORCE_GLOBAL, full_max=fmg,
                                 plan={"strategy": "global", "lane_major": 1})
        P["gb_global_sm"] = Path(role, AGG4, gb, DENSE, L.PA_QF_FORCE_GLOBAL | L.PA_QF_NO_LANE_MAJOR, full_max=fmg,
                                 plan={"strategy": "global", "lane_major": 0})
        if role == "f":  # (the filter column at nb: the paths whose plan does not hang on a sparse filter)
            P = {k: v for k, v in P.items() if v.frac == DENSE}
        role_paths.update({"%s_%s" % (k, role): v for k, v in P.items()})


def _dense(role_paths):
    """The dense GROUP BY kernels (lds_dense): filter f, key g and dictionary value v at nb in turn; own and shared
    dictionaries. COUNT + SUM of an INT column packs into one word (the packed kernels and their JIT)."""
    # full regime: the kernel keeps its value tables and the waves' packed rows in LDS (pa_plan.hip plan_gdense): own
    # dictionaries of v up to 2^13 values, shared 2^16; keys up to 2 * 2^8 (own) or 2^9 (shared)
    for role in ("f", "g", "v"):
        for shared in (False, True):
            fm = {"f": 16, "g": 9 if shared else 8, "v": 16 if shared else 13}[role]
            sfx = "%s_%s" % (role, "shared" if shared else "own")
            kw = dict(group_by=("g",), frac=DENSE, vtype="INT", shared=shared, full_max=fm)
            d = {"strategy": "lds_dense"}
            P = {}
            P["gd_step"] = Path(role, AGG4, flags=L.PA_QF_NO_GDENSE_LM | L.PA_QF_NO_REG_STAGE,
                                plan=dict(d, variant=("gdense4", "gdense8", "gdense12"), dense_packed=0), **kw)
            P["gd_lm_unpacked"] = Path(role, CNT_SUM, flags=L.PA_QF_NO_GD_PACK, plan=dict(d, variant=_lm, dense_packed=0), **kw)
            P["gd_lm_packed"] = Path(role, CNT_SUM, flags=L.PA_QF_NO_JIT, plan=dict(d, variant=_lm, dense_packed=1), **kw)
            # (the kernel hiprtc compiles for the query's widths: 0.2 s per case)
            P["gd_jit"] = Path(role, CNT_SUM, plan=dict(d, variant=_lm, dense_packed=2), **kw)
            if shared:  # register-staged tiles need every segment to share the LDS tables
                P["gd_reg_stage"] = Path(role, AGG4, flags=L.PA_QF_NO_GDENSE_LM,
                                         plan=dict(d, variant=("gdense_rs12", "gdense_rs8"), dense_packed=0), **kw)
            role_paths.update({"%s_%s" % (k, sfx): v for k, v in P.items()})


def _partitioned(role_paths):
    """A key space too large for LDS accumulators (g x k: 48 x 600 keys with own dictionaries): the partitioned plan's
    count + emit passes, its count-free emit (24 x 300 keys of shared dictionaries), and the global plan it replaces;
    keys g, k and value v at nb in turn."""
    for role in ("g", "k", "v"):
        fm = {"g": 10, "k": 12, "v": FULL_V}[role]
        gb = ("g", "k")
        part = {"strategy": "partitioned", "partition_keys": lambda n: n > 0}
        P = {}
        P["part_count_emit"] = Path(role, AGG4, gb, DENSE, L.PA_QF2_NO_COUNT_FREE, full_max=fm,
                                    plan=dict(part, count_free_emit=0))
        # (the count-free emit takes dictionaries every segment shares: pa_jit.hip pve_plan; its kernels are compiled
        # by hiprtc per width, 0.3 s a case)
        P["part_count_free_shared"] = Path(role, AGG4, gb, DENSE, shared=True, full_max=fm,
                                           plan=dict(part, count_free_emit=1))
        P["part_off_global"] = Path(role, AGG4, gb, DENSE, L.PA_QF_NO_PARTITION, full_max=fm,
                                    plan={"strategy": "global", "partition_keys": 0})
        role_paths.update({"%s_%s" % (k, role): v for k, v in P.items()})
    # the filter column at nb under the count-free emit: the leaf's MSB-aligned windows (pve_jit.hip unpack<C, true>)
    role_paths["part_count_free_shared_f"] = Path(
        "f", AGG4, ("g", "k"), DENSE, shared=True, full_max=16,
        plan={"strategy": "partitioned", "partition_keys": lambda n: n > 0, "count_free_emit": 1})
    # the H stream: DISTINCTCOUNTHLLMV over the multi-value column at nb, next to the V stream
    role_paths["part_count_free_hll_m"] = Path(
        "m", (), kind="oracle", shared=True, full_max=12, plan=dict(strategy="partitioned", count_free_emit=2),
        sql="SELECT g, k, COUNT(*), SUM(v), DISTINCTCOUNTHLLMV(m) FROM t WHERE f BETWEEN {lo} AND {hi} GROUP BY g, k "
            "LIMIT 1000000 OPTION(numGroupsLimit=1000000)")


def _limit(role_paths):
    """numGroupsLimit binding (40 first-seen groups per segment; a 1-bit k still leaves 24 x 2 keys per segment): the prefix walk (limit_walk_kernel's
    column-major key loads) and the sorted form (the per-doc decode_global kernels); keys g and k at nb."""
    sql = ("SELECT g, k, COUNT(*), SUM(v) FROM t WHERE f BETWEEN {lo} AND {hi} GROUP BY g, k LIMIT 1000000 "
           "OPTION(numGroupsLimit=40)")
    for role in ("g", "k", "v"):
        fm = {"g": 10, "k": 12, "v": FULL_V}[role]
        role_paths["limit_walk_%s" % role] = Path(role, (), kind="oracle", sql=sql, full_max=fm,
                                                  plan={"limit_trimming": 2})
        role_paths["limit_sorted_%s" % role] = Path(role, (), kind="oracle", sql=sql, flags=L.PA_QF_NO_LIMIT_WALK,
                                                    full_max=fm, plan={"limit_trimming": 1})


def _hashed(role_paths):
    """A dictionary component at nb next to a raw column in the hashed key space: one-word keys (g + raw INT) and
    two-word keys (g + raw LONG + raw INT)."""
    for role in ("g", "v"):
        fm = FULL_G_GLOBAL if role == "g" else FULL_V
        role_paths["hashed_one_word_%s" % role] = Path(role, AGG4, ("g", "ri"), DENSE, full_max=fm,
                                                       plan={"strategy": "global", "variant": "global"},
                                                       attrs={"hashed": True, "key_words": 1})
        role_paths["hashed_two_words_%s" % role] = Path(role, AGG4, ("g", "rl", "ri"), DENSE, full_max=fm,
                                                        plan={"strategy": "global", "variant": "global"},
                                                        attrs={"hashed": True, "key_words": 2})


def _row_queries(role_paths):
    """Selection, distinct, filtered aggregations and expressions: the ORDER BY / key / operand column at nb, in the
    LDS and the global variant of each (selection has one)."""
    for role in ("g", "v"):
        fm = FULL_V if role == "v" else 10
        role_paths["select_%s" % role] = Path(
            role, (), kind="select", full_max=fm, plan={"strategy": "select"},
            sql="SELECT g, v, h FROM t WHERE f BETWEEN {lo} AND {hi} ORDER BY g DESC, v LIMIT 300")
    for role in ("g", "k"):
        for lds in (2, 0):
            role_paths["distinct_%s_%s" % ("lds" if lds else "global", role)] = Path(
                role, (), kind="distinct", full_max=8, tuning={"distinct_lds": lds},
                plan={"variant": "distinct_lds" if lds else "distinct_global"},
                sql="SELECT DISTINCT g, k FROM t WHERE f BETWEEN {lo} AND {hi} LIMIT 100000")
    for role in ("h", "v"):
        for lds in (1, 0):
            role_paths["filtered_%s_%s" % ("lds" if lds else "global", role)] = Path(
                role, (), kind="filtered", full_max=FULL_H if role == "h" else FULL_V, tuning={"filtered_lds": lds},
                plan={"variant": "filtered_lds" if lds else "filtered_global"},
                sql="SELECT g, COUNT(*) FILTER (WHERE h < 14), SUM(v) FILTER (WHERE h >= 14), MAX(v), "
                    "MIN(v) FILTER (WHERE h BETWEEN 7 AND 21) FROM t WHERE f BETWEEN {lo} AND {hi} GROUP BY g LIMIT 100000")
    for role in ("g", "v"):
        for lds in (1, 0):
            role_paths["expr_%s_%s" % ("lds" if lds else "global", role)] = Path(
                role, (), kind="expr", full_max=FULL_G if role == "g" else FULL_V, tuning={"expr_lds": lds},
                plan={"variant": "expr_lds" if lds else "expr_global"},
                sql="SELECT g, SUM(ADD(v, h)), MAX(SUB(v, g)), COUNT(*) FROM t WHERE f BETWEEN {lo} AND {hi} "
                    "GROUP BY g LIMIT 100000")


def _mv(role_paths):
    """The MV value stream (read through mv_off) at nb: filter leaves (ANY value for IN / ranges, ALL for NOT IN),
    COUNTMV / SUMMV / MINMV / MAXMV, and the MV column as a group key, per doc and partitioned."""
    kw = dict(kind="oracle", full_max=16)
    lane = {"strategy": "lane", "variant": "lane_dict", "lane_major": 1}   # (aggregation-only over the SV column v)
    lds = {"strategy": "lds", "variant": "lds", "lane_major": 1}
    role_paths["mv_filter_any_m"] = Path("m", (), sql="SELECT COUNT(*), SUM(v) FROM t WHERE m IN ({mset})", plan=lane, **kw)
    role_paths["mv_filter_range_m"] = Path("m", (), sql="SELECT COUNT(*), SUM(v) FROM t WHERE m BETWEEN {mlo} AND {mhi}",
                                           plan=lane, **kw)
    role_paths["mv_filter_all_m"] = Path("m", (), sql="SELECT g, COUNT(*), SUM(v) FROM t WHERE m NOT IN ({mnot}) "
                                         "GROUP BY g LIMIT 100000", plan=lds, **kw)
    role_paths["mv_aggregations_m"] = Path("m", (), sql="SELECT COUNTMV(m), SUMMV(m), MINMV(m), MAXMV(m), COUNT(*) FROM t "
                                           "WHERE f BETWEEN {lo} AND {hi}", plan=lds, **kw)
    gsql = ("SELECT m, COUNT(*), SUM(v), MAXMV(m) FROM t WHERE f BETWEEN {lo} AND {hi} GROUP BY m LIMIT 1000000 "
            "OPTION(numGroupsLimit=1000000)")
    # per doc, on LDS accumulators (up to 2 * 2^10 keys of COUNT + 3 slots in their 64 KiB) and on global ones
    role_paths["mv_group_by_lds_m"] = Path("m", (), sql=gsql, plan=lds, kind="oracle", full_max=10)
    role_paths["mv_group_by_global_m"] = Path("m", (), sql=gsql, flags=L.PA_QF_FORCE_GLOBAL,
                                              plan={"strategy": "global", "variant": "global"}, kind="oracle", full_max=12)
    role_paths["mv_group_by_partitioned_m"] = Path(
        "m", (), sql="SELECT m, k, COUNT(*), SUM(v) FROM t WHERE f BETWEEN {lo} AND {hi} GROUP BY m, k LIMIT 1000000 "
        "OPTION(numGroupsLimit=1000000)", plan={"strategy": "partitioned"}, kind="oracle", full_max=12)


def _stats(role_paths):
    """The statistics kernels over a leaf column at nb. pa_query_leaf_bitmaps (leaf_bitmap_kernel: one doc at a time)
    against numpy bitmaps; pa_query_filter_counts, whose leaf_bitmaps_batch_kernel builds the bitmaps lane-major for
    dictionary leaves (leaf_bitmap_tiles_lm -> leaf_lm<nb>; DICT_RANGE and DICT_SET of f) and in batches for MV leaves
    (leaf_bitmap_batch; m), against numpy counts: popcount(A), popcount(B) and popcount(A & B) for the leaf under test
    A and three other leaves B of every segment."""
    cnt = {"strategy": "lane", "variant": "lane_cnt", "lane_major": 1}
    role_paths["leaf_bitmaps_f"] = Path("f", (), kind="bitmaps", full_max=FULL_V, plan=cnt,
                                        sql="SELECT COUNT(*) FROM t WHERE f BETWEEN {lo} AND {hi}")
    role_paths["leaf_bitmaps_m"] = Path("m", (), kind="bitmaps", full_max=16, plan=cnt,
                                        sql="SELECT COUNT(*) FROM t WHERE m IN ({mset})")
    others = " OR g BETWEEN 0 AND 59 OR h BETWEEN 0 AND 13 OR k BETWEEN 100 AND 299"
    lane = {"strategy": "lane"}
    role_paths["filter_counts_range_f"] = Path("f", (), kind="counts", full_max=FULL_V, plan=lane,
                                               sql="SELECT COUNT(*) FROM t WHERE f BETWEEN {lo} AND {hi}" + others)
    role_paths["filter_counts_set_f"] = Path("f", (), kind="counts", full_max=FULL_V, plan=lane,
                                             sql="SELECT COUNT(*) FROM t WHERE f IN ({fset})" + others)
    role_paths["filter_counts_m"] = Path("m", (), kind="counts", full_max=16, plan=lane,
                                         sql="SELECT COUNT(*) FROM t WHERE m IN ({mset})" + others)


PATHS = {}
_agg(PATHS)
_group_by(PATHS)
_dense(PATHS)
_partitioned(PATHS)
_limit(PATHS)
_hashed(PATHS)
_row_queries(PATHS)
_mv(PATHS)
_stats(PATHS)

# (path, nb) left out -> the planner line or documented limit that excludes it. All lie below the natural width
# of a group key, where the key column holds 2^nb values only and the table's key space no longer needs the path.
EXCLUDED = {}
_FITS_LDS = ("key space of 48 x 2 * 2^nb keys fits the LDS strategy's 64 KiB of accumulators "
             "(pa_plan_kernels.hip plan_strategy: P.lds_acc <= 64 * 1024 takes STRAT_LDS before partitioning)")
_FITS_DENSE = ("key box of at most kGdMaxKeys keys over shared dictionaries: the dense GROUP BY kernel takes the query "
               "(pa_plan.hip plan_gdense, before the partitioned plan)")
for _nb in range(1, 5):
    EXCLUDED[("part_count_emit_k", _nb)] = _FITS_LDS
    EXCLUDED[("part_off_global_k", _nb)] = _FITS_LDS
    EXCLUDED[("part_count_free_shared_g", _nb)] = _FITS_DENSE
for _nb in range(1, 9):
    EXCLUDED[("part_count_free_shared_k", _nb)] = _FITS_DENSE
EXCLUDED[("mv_group_by_partitioned_m", 1)] = _FITS_LDS.replace("48 x 2 * 2^nb", "4 x 600")


def regimes_of(path, nb):
    """The regimes one (path, nb) case runs: the sweep regime, and the full regime where the path's tables allow."""
    p = PATHS[path]
    out = [W.base_regime(p.role, nb)]
    if W.NATURAL[p.role][0] < nb <= p.full_max:
        out.append("full")
    return out


def _cases():
    out = [(name, nb) for name in PATHS for nb in W.WIDTHS if (name, nb) not in EXCLUDED]
    # cases of one role and width next to each other: the module keeps that group's tables (and their GPU segments)
    out.sort(key=lambda c: (_group_key(c[0], c[1]), c[0]))
    return out


def _group_key(path, nb):
    p = PATHS[path]
    return (p.role, p.vtype, p.shared, nb)


CASES = _cases()
_CACHE = {}  # the tables of the last (role, value type, shared, nb): regime -> (Table, GPU segments, {query: reference})


def _release_tables():
    for _, gs, _ in _CACHE.get("tables", {}).values():
        for g in gs:
            g.close()
    _CACHE.clear()


def _table(case):
    path, nb, regime = case
    group = _group_key(path, nb)
    if _CACHE.get("group") != group:
        _release_tables()
        _CACHE.update(group=group, tables={})
    if regime not in _CACHE["tables"]:
        role, vtype, shared, _ = group
        t = W.build_table(role, nb, regime, vtype=vtype, shared=shared)
        _CACHE["tables"][regime] = (t, [GpuSegment(s) for s in t.segments], {})
    return _CACHE["tables"][regime]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _release_tables()


def plan_mismatches(p, ex, gs):
    """(plan, [(field, value)] that are not the path's) of a prepared executor."""
    plan = ex.stats()["plan"]
    bad = []
    for k, want in p.plan.items():
        have = plan[k]
        ok = want(have) if callable(want) else (have in want if isinstance(want, tuple) else have == want)
        if not ok:
            bad.append((k, have))
    for c, want in p.staged.items():
        have = int(L.lib().pa_query_column_staged(ex.handle, gs[0].column_ids[c]))
        if have != want:
            bad.append(("staged:" + c, have))
    bad += [(a, getattr(ex, a)) for a, want in p.attrs.items() if getattr(ex, a) != want]
    return plan, bad


def _mv_literals(t):
    """Values of m for its leaves: the first, the last and the 0101 / 1010 ids' values of both segments' dictionaries
    (IN / NOT IN), and a range over the lower 60 % of the ids."""
    card = t.card("m")
    vals = sorted({int(seg.column("m").dictionary[i]) for seg in t.segments for i in W.special_ids(card).tolist() + [card // 3]})
    # (NOT IN: the first and one middle id only, so that docs remain even when m holds two values)
    nots = sorted({int(seg.column("m").dictionary[i]) for seg in t.segments for i in (0, card // 3)})
    return {"mset": ", ".join(map(str, vals)), "mnot": ", ".join(map(str, nots)), "mlo": 0,
            "mhi": 4 * max(1, int(card * 0.6)) - 1}


def _f_set(t):
    """Values of f for an IN list: those of the special ids and of every third id below 90, in both segments'
    dictionaries (a DICT_SET leaf once the ids are not one run)."""
    card = t.card("f")
    ids = sorted(set(W.special_ids(card).tolist()) | set(range(0, min(card, 90), 3)))
    return sorted({int(seg.column("f").dictionary[i]) for seg in t.segments for i in ids})


def _query(p, t):
    lo, hi = t.filter_bounds(p.frac)
    mv = _mv_literals(t) if "m" in t.segments[0].columns else {}
    return parse_sql(p.sql.format(lo=lo, hi=hi, fset=", ".join(map(str, _f_set(t))), **mv))


def _result(res, grouped):
    return (res.num_docs_scanned, res.groups if grouped else res.row)


def _run_numpy(p, t, gs, refs):
    where = None if p.frac is None else t.filter_bounds(p.frac)
    rk = (p.aggs, p.group_by, where)
    if rk not in refs:
        refs[rk] = W.reference(t, list(p.aggs), p.group_by, where)
    q = parse_sql(W.sql(list(p.aggs), p.group_by, where))
    ex = GpuQueryExecutor(q, gs, flags=p.flags, tuning=dict(GRID, **p.tuning))
    try:
        plan, bad = plan_mismatches(p, ex, gs)
        ex.execute()
        res = ex.fetch(execution_stats=False)
    finally:
        ex.close()
    return plan, bad, _result(res, p.group_by), refs[rk]


def _run_oracle(p, t, gs, refs):
    """The oracle's result (pinned against numpy at every width by test_bit_widths_oracle.py) as the reference."""
    import oracle
    q = _query(p, t)
    if (p.sql, p.frac) not in refs:
        r = oracle.run_query(q, t.segments)
        refs[(p.sql, p.frac)] = (r.num_docs_scanned, (r.groups if q.group_by else r.row, r.num_groups_limit_reached))
    ex = GpuQueryExecutor(q, gs, flags=p.flags, tuning=dict(GRID, **p.tuning))
    try:
        plan, bad = plan_mismatches(p, ex, gs)
        ex.execute()
        res = ex.fetch(execution_stats=False)
    finally:
        ex.close()
    got = (res.num_docs_scanned, (res.groups if q.group_by else res.row, res.num_groups_limit_reached))
    return plan, bad, got, refs[(p.sql, p.frac)]


def _run_filtered(p, t, gs, refs):
    import filtered_ref as FR
    q = _query(p, t)
    if (p.sql, p.frac) not in refs:
        r = FR.numpy_eval(q, t.segments)
        refs[(p.sql, p.frac)] = (r.num_docs_scanned, r.groups)
    ex = GpuQueryExecutor(q, gs, flags=p.flags, tuning=dict(GRID, **p.tuning))
    try:
        plan, bad = plan_mismatches(p, ex, gs)
        ex.execute()
        res = ex.fetch(execution_stats=False)
    finally:
        ex.close()
    return plan, bad, (res.num_docs_scanned, res.groups), refs[(p.sql, p.frac)]


def _run_expr(p, t, gs, refs):
    import transform_ref as TR
    q = _query(p, t)
    if (p.sql, p.frac) not in refs:
        r, _ = TR.reference(q, t.segments)  # (the materialised query's row: this query's aggregations come first)
        refs[(p.sql, p.frac)] = (r.num_docs_scanned, {k: v[:len(q.aggregations)] for k, v in r.groups.items()})
    ex = GpuQueryExecutor(q, gs, flags=p.flags, tuning=dict(GRID, **p.tuning))
    try:
        plan, bad = plan_mismatches(p, ex, gs)
        ex.execute()
        res = ex.fetch(execution_stats=False)
    finally:
        ex.close()
    return plan, bad, (res.num_docs_scanned, res.groups), refs[(p.sql, p.frac)]


def _run_select(p, t, gs, refs):
    import selection_ref as SR
    from pinot_amd.engine import SelectionExecutor
    q = _query(p, t)
    if (p.sql, p.frac) not in refs:
        r = SR.run(q, t.segments)
        n = min(int(q.limit), len(r.rows))
        refs[(p.sql, p.frac)] = (n, [r.segments[:n].tolist(), r.docs[:n].tolist(), r.keys[:n].tolist(), r.rows[:n]])
    ex = SelectionExecutor(q, gs, flags=p.flags, tuning=dict(GRID, **p.tuning))
    try:
        plan, bad = plan_mismatches(p, ex, gs)
        res = ex.run()
    finally:
        ex.close()
    got = (len(res.rows), [res.segments.tolist(), res.docs.tolist(), res.keys.tolist(), [list(r) for r in res.rows]])
    exp = refs[(p.sql, p.frac)]
    return plan, bad, got, (exp[0], exp[1][:3] + [[list(r) for r in exp[1][3]]])


def _run_distinct(p, t, gs, refs):
    import distinct_ref as DR
    from pinot_amd.engine import DistinctExecutor
    q = _query(p, t)
    if (p.sql, p.frac) not in refs:
        r = DR.completed_server(q, t.segments, force_scan=True)
        refs[(p.sql, p.frac)] = (r.present, [list(x) for x in r.rows])
    ex = DistinctExecutor(q, gs, flags=p.flags, tuning=dict(GRID, **p.tuning), force_scan=True)
    try:
        plan, bad = plan_mismatches(p, ex, gs)
        res = ex.run()
    finally:
        ex.close()
    return plan, bad, (res.present, [list(x) for x in res.rows]), refs[(p.sql, p.frac)]


def _run_bitmaps(p, t, gs, refs):
    """Every doc's leaf bit of both segments against numpy over the generated ids."""
    q = _query(p, t)
    if (p.sql, p.frac) not in refs:
        masks = []
        for si, seg in enumerate(t.segments):
            if p.role == "f":
                lo, hi = t.filter_bounds(p.frac)
                fv = t.values(si, "f")
                masks.append(((fv >= lo) & (fv <= hi)).tolist())
            else:
                want = {int(x) for x in _mv_literals(t)["mset"].split(", ")}
                masks.append([bool(want & set(r.tolist())) for r in t.mv_values(si)])
        refs[(p.sql, p.frac)] = (sum(sum(m) for m in masks), masks)
    ex = GpuQueryExecutor(q, gs, flags=p.flags, tuning=dict(GRID, **p.tuning))
    try:
        plan, bad = plan_mismatches(p, ex, gs)
        ex.execute()
        res = ex.fetch(execution_stats=False)
        maps = [ex.leaf_bitmaps(si) for si in range(len(gs))]
    finally:
        ex.close()
    assert all(m.shape[0] == 1 for m in maps)
    assert res.row[0] == res.num_docs_scanned
    return plan, bad, (res.num_docs_scanned, [m[0].tolist() for m in maps]), refs[(p.sql, p.frac)]


def _run_counts(p, t, gs, refs):
    """pa_query_filter_counts: for every segment and every other leaf B, popcount(A), popcount(B), popcount(A & B) with A
    the leaf under test, against numpy masks over the generated ids."""
    from pinot_amd.engine import _flatten_filter
    q = _query(p, t)
    lo, hi = t.filter_bounds(p.frac)
    if (p.sql, p.frac) not in refs:
        per_seg = []
        for si, seg in enumerate(t.segments):
            if "fset" in p.sql:
                a = np.isin(t.values(si, "f"), _f_set(t))
            elif p.role == "f":
                fv = t.values(si, "f")
                a = (fv >= lo) & (fv <= hi)
            else:
                want = {int(x) for x in _mv_literals(t)["mset"].split(", ")}
                a = np.array([bool(want & set(r.tolist())) for r in t.mv_values(si)])
            gv, hv, kv = t.values(si, "g"), t.values(si, "h"), t.values(si, "k")
            per_seg.append({p.role: a, "g": (gv >= 0) & (gv <= 59), "h": (hv >= 0) & (hv <= 13),
                            "k": (kv >= 100) & (kv <= 299)})
        union = sum(int((m[p.role] | m["g"] | m["h"] | m["k"]).sum()) for m in per_seg)
        counts = [[int(m[p.role].sum()), int(m[c].sum()), int((m[p.role] & m[c]).sum())] for m in per_seg for c in "ghk"]
        refs[(p.sql, p.frac)] = (union, counts)
    ex = GpuQueryExecutor(q, gs, flags=p.flags, tuning=dict(GRID, **p.tuning))
    try:
        plan, bad = plan_mismatches(p, ex, gs)
        leaves = []
        _flatten_filter(ex.query.filter, leaves, [])
        where = {pred.column: i for i, pred in enumerate(leaves)}
        assert sorted(where) == sorted({p.role, "g", "h", "k"}) and len(leaves) == 4, leaves
        if "fset" in p.sql and t.card("f") >= 8 and ex.spec.leaves[where["f"]].kind != L.PA_LEAF_DICT_SET:
            bad.append(("leaf kind", ex.spec.leaves[where["f"]].kind))
        ex.execute()
        res = ex.fetch(execution_stats=False)
        reqs = [(si, where[p.role], where[c]) for si in range(len(gs)) for c in "ghk"]
        segs = np.array([r[0] for r in reqs], dtype=np.int32)
        progs = np.zeros((len(reqs), 2, L.PA_BIT_PROG_MAX), dtype=np.int32)
        for r, (_, la, lb) in enumerate(reqs):
            progs[r, 0, 0], progs[r, 1, 0] = la, lb
        lengths = np.ones(2 * len(reqs), dtype=np.int32)
        out = np.zeros(4 * len(reqs), dtype=np.int64)
        L.check(L.lib().pa_query_filter_counts(ex.handle, len(reqs), segs.ctypes.data, progs.ctypes.data,
                                               lengths.ctypes.data, out.ctypes.data, None), "pa_query_filter_counts")
    finally:
        ex.close()
    assert res.row[0] == res.num_docs_scanned
    return plan, bad, (res.num_docs_scanned, out.reshape(-1, 4)[:, :3].tolist()), refs[(p.sql, p.frac)]


RUNNERS = {"counts": _run_counts, "numpy": _run_numpy, "oracle": _run_oracle, "filtered": _run_filtered, "expr": _run_expr,
           "select": _run_select, "distinct": _run_distinct, "bitmaps": _run_bitmaps}


def run_case(case):
    """(plan, what of it is not the path's, got, expected) of one case; got / expected: (a count, the result)."""
    p = PATHS[case[0]]
    t, gs, refs = _table(case)
    return RUNNERS[p.kind](p, t, gs, refs)


def first_difference(got, exp):
    if got[0] != exp[0]:
        return "numDocsScanned %r, expected %r" % (got[0], exp[0])
    if isinstance(exp[1], dict):
        if set(got[1]) != set(exp[1]):
            return "group keys differ: %r" % sorted(set(got[1]) ^ set(exp[1]))[:6]
        for k in sorted(exp[1]):
            if got[1][k] != exp[1][k]:
                return "group %r: %r, expected %r" % (k, got[1][k], exp[1][k])
        return None
    return None if got[1] == exp[1] else "row %r, expected %r" % (got[1], exp[1])


@pytest.mark.parametrize("path,nb", CASES, ids=["%s-%d" % c for c in CASES])
def test_width(path, nb):
    for regime in regimes_of(path, nb):
        plan, bad, got, exp = run_case((path, nb, regime))
        assert not bad, "%s nb=%d %s: plan %s is not the path's: %s" % (path, nb, regime, plan, bad)
        assert exp[0] > 0
        diff = first_difference(got, exp)
        assert diff is None, "%s nb=%d %s: %s (plan %s)" % (path, nb, regime, diff, plan)


def test_every_path_covers_every_width():
    """One case per path and nb in 1..31, less only EXCLUDED's entries."""
    assert set(CASES) | set(EXCLUDED) == {(n, nb) for n in PATHS for nb in W.WIDTHS}
    assert not set(CASES) & set(EXCLUDED)


# The direct key space holds one accumulator row per dictId: 2^nb rows. Up to 24 bits (a 128 MiB COUNT section) a case
# runs in well under a second; 25..27 bits (256 MiB .. 1 GiB per section, the reset and the fetch's count pass over all
# of it) are left out; from 28 bits the planner hashes (kDirectMaxKeys = 2^27, pa_host.h) and the table follows the docs.
CAPI_DIRECT_LEFT_OUT = (25, 26, 27)


@pytest.mark.parametrize("nb", [nb for nb in W.WIDTHS if nb not in CAPI_DIRECT_LEFT_OUT])
def test_string_group_by_through_capi(nb):
    """Raw C-ABI use: GROUP BY over an nb-bit STRING column without dictionary values, whose ids use all nb bits (0,
    2^nb - 1, 0101.., 1010.. at the planted docs). The keys are the dictIds, so the top bits of the wide widths reach a
    group key without a dictionary of that size: direct key space up to 27 bits, hashed from 28. Two segments; counts
    per dictId against numpy."""
    from pinot_amd.segment import pack_bits
    lib = L.lib()
    card = (1 << nb) if nb < 31 else (1 << 31) - 1
    segs, ids_all, keep = [], [], []
    for si, n in enumerate(W.SEG_DOCS):
        ids = np.minimum(W.make_ids(np.random.default_rng([nb, si]), n, 1 << nb), card - 1)
        fwd = pack_bits(ids.astype(np.uint32), nb)
        seg = L.check_ptr(lib.pa_segment_create(n), "create")
        L.check(lib.pa_segment_add_sv_dict_column(seg, 0, fwd.ctypes.data, fwd.nbytes, nb, card, L.PA_STRING, None, None),
                "add")
        segs.append(seg)
        ids_all.append(ids)
        keep.append(fwd)
    spec = L.QuerySpec()
    spec.num_group_by = 1
    spec.group_by_columns[0] = 0
    spec.group_by_cardinality[0] = card
    spec.num_aggs = 1
    spec.aggs[0].type = L.PA_AGG_COUNT
    q = L.check_ptr(lib.pa_query_create(ctypes.byref(spec), len(segs)), "qcreate")
    try:
        L.check(lib.pa_query_set_tuning(q, b"scan_grid", GRID["scan_grid"]), "tuning")
        for si, seg in enumerate(segs):
            L.check(lib.pa_query_bind_segment(q, si, seg, (L.LeafParams * 1)(), (ctypes.c_void_p * 1)()), "bind")
        L.check(lib.pa_query_prepare(q), "prepare")
        hashed, shifts = ctypes.c_int32(), (ctypes.c_int32 * 1)()
        L.check(lib.pa_query_key_layout(q, ctypes.byref(hashed), shifts), "key_layout")
        assert hashed.value == (1 if nb >= 28 else 0) and shifts[0] == 0 and lib.pa_query_key_words(q) == 1
        L.check(lib.pa_query_execute(q, None), "execute")
        n = L.check(lib.pa_query_fetch(q, None, 0, None, None, None), "count")
        keys, counts, outs = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.float64)
        ptrs = (ctypes.c_void_p * 1)(outs.ctypes.data)
        assert L.check(lib.pa_query_fetch(q, None, n, keys.ctypes.data, counts.ctypes.data, ptrs), "fetch") == n
        assert lib.pa_query_matched_docs(q) == sum(W.SEG_DOCS)
    finally:
        lib.pa_query_destroy(q)
        for seg in segs:
            lib.pa_segment_destroy(seg)
    want_keys, want_counts = np.unique(np.concatenate(ids_all), return_counts=True)
    assert {0, card - 1} <= set(want_keys.tolist())
    order = np.argsort(keys[:n], kind="stable")
    assert keys[:n][order].tolist() == want_keys.tolist()
    assert counts[:n][order].tolist() == want_counts.tolist()
