// The per-query tuning table: every override of a planner decision, defined once. A query carries the values
// (pa_query::tune, set by pa_query_set_tuning before pa_query_prepare: tests and measurement only); nothing here is
// read from the process environment. X(name, default, lowest, highest, results_invalid): the default is what the
// planner does on its own (-1: it decides per query); a tuning marked results_invalid skips work in a kernel when it
// is not 0, so pa_query_results_invalid reports it and pa_query_fetch / pack_rows / merge_rows refuse the query.
#pragma once
#include <cstdint>
#include <cstring>

#define PA_TUNINGS(X)                                                                                                  \
  /* gdl_jit.hip (jit_plan): waves per workgroup, docs per lane, waves sharing one set of packed rows: only the       \
     candidates with this value stay (none left: the generic kernel). By default the most resident waves, then the    \
     larger tile, then private rows */                                                                                \
  X(gdl_w, -1, 8, 16, 0)                                                                                               \
  X(gdl_nd, -1, 8, 16, 0)                                                                                              \
  X(gdl_rs, -1, 1, 2, 0)                                                                                               \
  /* gdl_jit.hip: replicas of a packed row, rounded down to a power of two that fits the LDS (default: as many as     \
     fit, up to one per lane) */                                                                                      \
  X(gdl_rr, -1, 1, 64, 0)                                                                                              \
  /* gdl_jit.hip: tile images per wave, RING - 1 tiles in flight while one is walked (default 2) */                  \
  X(gdl_ring, -1, 2, 4, 0)                                                                                             \
  /* gdl_jit.hip JIT_DBG: 1 = stream the tiles only, 2 = + the filter, 3 = + keys and terms, no row atomics */       \
  X(gdl_dbg, 0, 0, 3, 1)                                                                                               \
  /* pve_jit.hip (pve_stream): docs per lane, 8 or 16 (default: H 8, a lane's run of MV values is half as long, 3.97  \
     vs 4.8 ms on configs[4]; V 16 unless 8 leave room for more resident waves) */                                    \
  X(pve_nd, -1, 8, 16, 0)                                                                                              \
  /* pve_jit.hip: records per bin, 16 or 32 (default 32, 16 only when 32 leave fewer than 8 waves: 16-record bins for \
     more resident waves measured slower, V 1.70 vs 1.33 ms at 12 vs 8 waves, H 4.37 vs 3.97 ms at 16 vs 12) */       \
  X(pve_bs, -1, 16, 32, 0)                                                                                             \
  /* pve_jit.hip: compacted put rounds through a queue of 512 records per wave, 0 / 1 (default: a V stream whose      \
     filter keeps less than half the docs; configs[2] 10 %: 0.409 vs 0.496 ms per 200M docs, on every doc 1.38 vs     \
     1.20 ms, H stream 5.26 vs 3.89 ms) */                                                                            \
  X(pve_q, -1, 0, 1, 0)                                                                                                \
  /* pve_jit.hip: tile images per wave of a V stream (default 2; the H stream and admission loads always keep two) */ \
  X(pve_ring, -1, 2, 4, 0)                                                                                             \
  /* pve_jit.hip H stream: 0 = one claim per value instead of one per run of a doc's values (default 1) */            \
  X(pve_hrun, -1, 0, 1, 0)                                                                                             \
  /* pve_jit.hip H stream: values per run (default: the column's most values per doc, up to 8) */                     \
  X(pve_hb, -1, 1, 8, 0)                                                                                               \
  /* pve_jit.hip PVE_DBG: 1 = records built but not put, 2 = full bins not stored */                                  \
  X(pve_dbg, 0, 0, 2, 1)                                                                                               \
  /* pass C (launch_part_agg): V partitions at 16 waves per workgroup, 0 / 1 (default: one-word records only;         \
     configs[2] pass C 505 -> 364 us, the all-docs line 1.185 -> 1.069 ms; three-word raw-value records stay at 8     \
     waves with two batches, configs[4] 775 vs 735 us) */                                                             \
  X(passc_v16, -1, 0, 1, 0)                                                                                            \
  /* numGroupsLimit walk (launch_limit_walk): 0 = the replay without its first-lane table, the path also taken when   \
     the table does not fit the LDS (default 1) */                                                                    \
  X(walk_tab, 1, 0, 1, 0)                                                                                              \
  /* bit set of DevQuery::debug_emit and GdSegPlan::pad (pa_gdense.h): parts of the emit pass / the dense walk        \
     skipped. Keeps the generic kernels: no gdl_jit, and the count + emit passes unless pve_dbg is set */             \
  X(debug_emit, 0, 0, 127, 1)                                                                                          \
  /* scan_kernel, lane-major: whole tiles of a single equality leaf ask pa_eq_any.h "any match in this lane?" on the  \
     stream words before the per-doc leaf, 0 / 1 on where legal: columns of up to kEqPrefilterMaxNb bits (default:  \
     only where the launch also streams nt, the one combination that measured a gain) */                              \
  X(eq_prefilter, -1, 0, 1, 0)                                                                                         \
  /* scan_kernel, lane-major hoisted loops: the staged columns' LDS-DMAs carry the nt cache policy, 0 / 1 (default:   \
     only when one launch stages more bytes than L2 + Infinity Cache hold, so a smaller table that is queried again    \
     keeps its cache hits) */                                                                                          \
  X(stream_nt, -1, 0, 1, 0)                                                                                            \
  /* eqs_jit.hip (eqs_plan): the direct scan of one equality compiled per query shape, 0 never / 1 wherever the shape \
     fits (default: only behind a dictionary of at least 4096 values, where surviving docs are rare) */               \
  X(eq_jit, -1, 0, 1, 0)                                                                                               \
  /* eqs_jit.hip JIT_DBG: 1 = stream the tiles only, through the same (nt) DMAs and counted waits */                  \
  X(eqs_dbg, 0, 0, 1, 1)                                                                                               \
  /* workgroups of the non-partitioned scan launch (default: one wave per tile up to the resident workgroups). A      \
     small grid gives every wave several tiles of a small table, so tests reach the hoisted steady-state loops */      \
  X(scan_grid, -1, 1, 4096, 0)                                                                                         \
  /* pa_query_reset as one kernel launch instead of memsets + one fill per MIN / MAX / KEYS section, 0 / 1 (default:  \
     accumulator blocks up to kResetFusedMaxBytes) */                                                                  \
  X(reset_fused, -1, 0, 1, 0)                                                                                          \
  /* selection (STRAT_SELECT): bound in MiB of the scan waves' candidate block (waves x CAP x 16 bytes); the launch's \
     grid shrinks until the block fits. The default of 256 is NOT measured: it is one Infinity Cache's worth */       \
  X(select_scratch_mib, 256, 1, 16384, 0)                                                                              \
  /* selection: candidates per scan wave (CAP), K + 1 .. max(2 K, 128) (checked at prepare; default: that maximum).    \
     A small CAP makes small tables reach the in-place compaction */                                                  \
  X(select_cap, -1, 2, 131072, 0)                                                                                      \
  /* distinct (STRAT_DISTINCT_LDS): 0 = never the workgroup-private LDS bitmap, 1 = the planner's choice (default:    \
     the LDS bitmap when it fits next to the tile ring without costing resident workgroups), 2 = whenever it fits */   \
  X(distinct_lds, 1, 0, 2, 0)                                                                                          \
  /* filtered aggregations: 0 = device-scope atomics (STRAT_FILTERED), 1 = the workgroup-private LDS accumulators       \
     (STRAT_FILTERED_LDS) whenever they fit next to a tile ring (default: when they take at most 64 KiB and the lanes'  \
     union is dense, STRAT_LDS's rule) */                                                                               \
  X(filtered_lds, -1, 0, 1, 0)                                                                                         \
  /* transform expressions: 0 = device-scope atomics (STRAT_EXPR), 1 = the workgroup-private LDS accumulators           \
     (STRAT_EXPR_LDS) whenever the key space is direct and they fit next to a tile ring (default: when they take at    \
     most 64 KiB and the matching docs are dense, STRAT_LDS's rule) */                                                  \
  X(expr_lds, -1, 0, 1, 0)                                                                                             \
  /* hashed key spaces: the slot table holds at most this many slots (rounded down to a power of two; default: twice   \
     the keys that can exist, up to 2^28). A small cap lets a small table reach the group-key table overflow report */  \
  X(hash_slots_cap, -1, 1024, 1 << 28, 0)                                                                              \
  /* FIRSTWITHTIME / LASTWITHTIME: 1 = the wide form (two scan launches) for every raw time column, 0 = the packed     \
     form, refused at prepare where the time range does not fit beside the row (default: packed wherever it fits). A     \
     dictionary time column is always packed. Lets small tables reach the wide form */                                 \
  X(time_rows_wide, -1, 0, 1, 0)                                                                                       \
  /* FIRSTWITHTIME / LASTWITHTIME: 0 = device-scope atomics (STRAT_TROW), 1 = the workgroup-private LDS accumulators    \
     (STRAT_TROW_LDS) whenever they fit next to a tile ring (default: when they take at most 64 KiB and the matching    \
     docs are dense, STRAT_LDS's rule; PA_QF_FORCE_LDS / PA_QF_FORCE_GLOBAL act as on STRAT_LDS) */                    \
  X(time_rows_lds, -1, 0, 1, 0)                                                                                        \
  /* VAR_POP / STDDEV / COVAR: 0 = device-scope atomics (STRAT_MOM), 1 = the workgroup-private LDS accumulators         \
     (STRAT_MOM_LDS) whenever they fit next to a tile ring (default: when they take at most 64 KiB and the matching     \
     docs are dense, STRAT_LDS's rule; PA_QF_FORCE_LDS / PA_QF_FORCE_GLOBAL act as on STRAT_LDS) */                    \
  X(moments_lds, -1, 0, 1, 0)

struct Tuning {
#define X(name, def, lo, hi, inv) int32_t name = def;
  PA_TUNINGS(X)
#undef X
};

struct TuningDef {
  const char* name;
  int32_t Tuning::*value;
  int32_t def, lo, hi;
  bool results_invalid;
};
inline constexpr TuningDef kTunings[] = {
#define X(name, def, lo, hi, inv) {#name, &Tuning::name, def, lo, hi, inv != 0},
    PA_TUNINGS(X)
#undef X
};

inline const TuningDef* tuning_named(const char* name) {
  for (const TuningDef& d : kTunings)
    if (name && std::strcmp(d.name, name) == 0) return &d;
  return nullptr;
}

// the first tuning set that invalidates the query's results, or null
inline const char* tuning_invalidating(const Tuning& t) {
  for (const TuningDef& d : kTunings)
    if (d.results_invalid && t.*d.value != d.def) return d.name;
  return nullptr;
}
