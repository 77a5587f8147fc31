/*
 * pinot_amd.h — C-ABI of the MI355X-native segment query hot path.
 *
 * This is the drop-in boundary a Pinot server binds (Java FFM / JNI).
 * Everything above it (QueryContext, PredicateEvaluator, Dictionary, DataTable building,
 * broker reduce) stays in the host language; everything below it runs as hand-written HIP
 * on gfx950. Plain pointers and sizes only — no torch, no C++ types.
 *
 * Reference interfaces replaced (all paths relative to /root/reference):
 *
 *  pa_segment_add_sv_dict_column
 *      replaces the device-side role of
 *      pinot-segment-local/.../readers/forward/FixedBitSVForwardIndexReaderV2.java:38 (ctor over the
 *      PinotDataBuffer) and io/reader/impl/FixedBitIntReader.java:51 (getReader): the caller passes the
 *      forward-index bytes exactly as written by FixedBitSVForwardIndexWriter (big-endian, MSB-first,
 *      io/util/PinotDataBitSet.java:80 layout) and the dictionary values
 *      (segment-spi/.../index/reader/Dictionary.java getLongValue/getDoubleValue).
 *  pa_segment_add_mv_dict_column
 *      replaces readers/forward/FixedBitMVForwardIndexReader.java:56 (chunk offsets + row-start bitmap
 *      + bit-packed values, same bytes).
 *  pa_segment_add_raw_column
 *      replaces the raw (no-dictionary) fixed-width forward index readers
 *      (readers/forward/FixedByteChunkSVForwardIndexReader.java) — values are passed decoded.
 *  pa_query_* (spec, bind, execute, fetch)
 *      replaces, for one segment set on one GPU, the per-segment operator chain
 *        pinot-core/.../operator/filter/ScanBasedFilterOperator.java + dociditerators/SVScanDocIdIterator.java:76
 *        operator/filter/BitmapBasedFilterOperator.java, AndFilterOperator.java, OrFilterOperator.java,
 *        NotFilterOperator.java (the filter tree, evaluated in dictId space from
 *        operator/filter/predicate/{Range,In,Equals,NotIn,NotEquals}PredicateEvaluatorFactory.java ranges / matching-dictId sets),
 *        operator/query/AggregationOperator.java and operator/query/GroupByOperator.java:84
 *        (query/aggregation/groupby/DefaultGroupByExecutor.java:140 process(),
 *         DictionaryBasedGroupKeyGenerator.java:233 raw-key generation,
 *         aggregation/function/{Count,Sum,Min,Max,DistinctCountHLL}AggregationFunction.java
 *         aggregateGroupBySV / aggregate),
 *      and the in-server merge of those partial results
 *        operator/combine/AggregationCombineOperator.java, GroupByCombineOperator.java:110
 *      (segments of one GPU accumulate into ONE table-wide key space, so no per-segment merge is needed).
 *  pa_query_fetch_histogram / pa_query_percentiles (PA_AGG_VALUE_HISTOGRAM)
 *      replace aggregation/function/PercentileAggregationFunction.java and PercentileMVAggregationFunction.java:
 *      aggregate / aggregateGroupBySV / aggregateGroupByMV (every value into a DoubleArrayList) become per-group value
 *      histograms inside the scan, extractAggregationResult / extractGroupByResult the compacted (value id, count)
 *      pairs, extractFinalResult (sort + index at the percentile's rank) a rank select over the bins on the GPU.
 *  pa_query_fetch_trimmed
 *      replaces, for a direct key space, the server's group trim: data/table/IndexedTable.java:149 (finish) with
 *      data/table/TableResizer.java:187-238 (resizeRecordsMap: the top `trim` records under the ORDER BY comparator) at
 *      the capacity of GroupByUtils.getTableCapacity / operator/combine/GroupByCombineOperator.java:63-73 — an MSB
 *      radix select over order words in HBM, then a gather of the kept groups' rows only.
 *  pa_query_fetch_time_rows / pa_query_time_row_form (PA_AGG_LAST_ROW_BY_TIME / PA_AGG_FIRST_ROW_BY_TIME)
 *      replace aggregation/function/LastWithTimeAggregationFunction.java and FirstWithTimeAggregationFunction.java with
 *      their per-type subclasses ({First,Last}{Int,Long,Float,Double,String}ValueWithTimeAggregationFunction.java;
 *      factory cases AggregationFunctionFactory.java:224-252 and :324-350): aggregate / aggregateGroupBySV (the doc with
 *      time >= / <= the best so far takes over, :112,147,196 / :111,147,200) and the in-server merge (:223 / :227) become
 *      one 64-bit max per group inside the scan; extractAggregationResult / extractGroupByResult (the ValueTimePair)
 *      the winning (segment, doc) and the cells a finish kernel reads there.
 *  pa_query_set_moments / pa_query_fetch_moments / pa_query_moments_form (PA_AGG_MOMENTS)
 *      replace aggregation/function/VarianceAggregationFunction.java (VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP) and
 *      CovarianceAggregationFunction.java (COVAR_POP / COVAR_SAMP; factory cases AggregationFunctionFactory.java:413-427):
 *      aggregate / aggregateGroupBySV (VarianceTuple.apply per doc; the raw sums of CovarianceAggregationFunction.java:100-108)
 *      and the in-server merge become moment sums kept per group inside the scan — exact integers for int32-range
 *      INT / LONG columns, pivoted power sums in double otherwise; extractAggregationResult / extractGroupByResult the
 *      VarianceTuple (count, sum, m2) / CovarianceTuple (sumX, sumY, sumXY, count) columns a finish kernel writes.
 *  pa_query_set_selection / pa_query_bind_order_remap / pa_query_fetch_selection
 *      replace, for one segment set on one GPU, operator/query/SelectionOnlyOperator.java,
 *      operator/query/SelectionOrderByOperator.java:108-112 (the comparator), :139-188 (every ordered expression
 *      fetched for every matching doc into a bounded priority queue), :193-322 (the rest of the row fetched for the
 *      rows kept) and operator/combine/SelectionOrderByCombineOperator.java (the segments' queues merged): one fused
 *      filter + top-K scan over every bound segment, then a select + sort of the candidates and a gather of the cells.
 *  pa_query_set_distinct / pa_query_fetch_distinct
 *      replace operator/query/DistinctOperator.java:55-84 with the dictionary-based executors
 *      (query/distinct/dictionary/DictionaryBasedMultiColumnDistinct{Only,OrderBy}Executor.java) and
 *      operator/combine/DistinctCombineOperator.java: one fused filter + key-presence bitmap scan over every bound
 *      segment, then a rank / order pass over the bits.
 *  pa_query_accumulators / layout
 *      exposes the device accumulators so the cross-GPU merge of partial aggregates runs as an RCCL
 *      reduce (SUM for COUNT/SUM, MIN, MAX, MAX for HLL registers) — the multi-GPU analogue of
 *      GroupByCombineOperator's IndexedTable upsert/merge.
 *
 * Error convention: functions returning int return 0 on success and a negative PA_E* code on error;
 * pa_last_error() returns a thread-local message. Functions returning pointers return NULL on error.
 */
#ifndef PINOT_AMD_H_
#define PINOT_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PA_ABI_VERSION 5

/* limits of one query shape */
#define PA_MAX_LEAVES 16
#define PA_MAX_OPS 48
#define PA_MAX_GROUP_BY 8
#define PA_MAX_AGGS 16
#define PA_MAX_ORDER_BY 8         /* ORDER BY columns of a selection */
#define PA_MAX_SELECT_COLUMNS 64  /* output columns of a selection */
#define PA_MAX_SELECT_ROWS 65536  /* rows a selection keeps (offset + limit) */
#define PA_MAX_AGG_FILTERS 8      /* distinct aggregation filters (AGG(x) FILTER (WHERE ...)) of one query */
#define PA_MAX_EXPRS 8            /* transform expressions (programs) of one query */
#define PA_MAX_EXPR_OPS 16        /* three-address operations of one expression program */
#define PA_MAX_EXPR_REGS 8        /* value registers of an expression program */
#define PA_MAX_EXPR_COLUMNS 8     /* distinct operand columns of all expressions of one query */

/* error codes */
#define PA_OK 0
#define PA_EINVAL (-1)
#define PA_EHIP (-2)
#define PA_ENOMEM (-3)
#define PA_EUNSUPPORTED (-4)

/* stored value types: org.apache.pinot.spi.data.FieldSpec.DataType#getStoredType */
#define PA_INT 0
#define PA_LONG 1
#define PA_FLOAT 2
#define PA_DOUBLE 3
#define PA_STRING 4
#define PA_BYTES 5

/* filter leaf kinds (how a predicate is evaluated on the GPU; resolution into dictId space happens in
 * the host's PredicateEvaluator exactly as in the reference) */
#define PA_LEAF_DICT_RANGE 0 /* lo <= dictId < hi   (SortedDictionaryBasedRangePredicateEvaluator, EQ)   */
#define PA_LEAF_DICT_SET 1   /* bit dictId of lut set (IN / NOT IN / unsorted range matching-dictId set)  */
#define PA_LEAF_RAW_RANGE 2  /* ilo<=v<=ihi (INT/LONG) or dlo<=v<=dhi (FLOAT/DOUBLE) on a raw column       */
#define PA_LEAF_MV_DICT_RANGE 3 /* MV column: any value with lo <= dictId < hi (MVScanDocIdIterator)      */
#define PA_LEAF_MV_DICT_SET 4   /* MV column: any value whose bit is set in lut                            */
#define PA_LEAF_RAW_SET 5       /* raw column: v is one of the leaf's num_values values (IN / NOT IN on a no-dictionary
                                   column: RawValueBasedInPredicateEvaluatorFactory.java's value sets), any list size */

/* postfix filter program opcodes; PA_OP_LEAF carries the leaf index in bits 8..15 */
#define PA_OP_LEAF 0
#define PA_OP_AND 1
#define PA_OP_OR 2
#define PA_OP_NOT 3

/* aggregation types (AggregationFunctionType) */
#define PA_AGG_COUNT 0
#define PA_AGG_SUM 1
#define PA_AGG_MIN 2
#define PA_AGG_MAX 3
#define PA_AGG_DISTINCTCOUNTHLL 4
#define PA_AGG_COUNT_MV 5 /* COUNTMV: number of values of an MV column (AVGMV = SUM over an MV column / COUNTMV) */
#define PA_AGG_DISTINCTCOUNT 6 /* exact DISTINCTCOUNT over a dictionary-encoded column: per group, one presence byte per
                                  table-wide value id of the column (pa_agg_spec.num_values of them; segment dictIds are
                                  mapped by pa_query_bind_value_remap) — the value set of DistinctCountAggregationFunction
                                  (BaseDistinctAggregateAggregationFunction) as a bitmap over the table's values */
#define PA_AGG_VALUE_HISTOGRAM 7 /* per group, how many times each value of a dictionary-encoded column was aggregated:
                                    one 64-bit count per table-wide value id (pa_agg_spec.num_values of them, segment
                                    dictIds mapped by pa_query_bind_value_remap, both as for DISTINCTCOUNT). The bins in
                                    ascending value order are PercentileAggregationFunction's DoubleArrayList as a multiset
                                    (aggregate / aggregateGroupBySV add every value; merge is addAll = bin-wise addition);
                                    over a multi-value column every value of the doc counts
                                    (PercentileMVAggregationFunction). Direct key spaces only: pa_query_prepare fails with
                                    PA_EUNSUPPORTED over a hashed key space, and for a raw or STRING / BYTES column. Read
                                    with pa_query_fetch_histogram / pa_query_percentiles; pa_query_fetch writes nothing
                                    for it */
#define PA_AGG_LAST_ROW_BY_TIME 8  /* LASTWITHTIME: per group the doc with the greatest value of the time column
                                      `column_id` (an SV INT / LONG column, raw or dictionary-encoded in every bound
                                      segment). Within a segment docs are offered in docId order and a doc with time >=
                                      the best takes over (LastWithTimeAggregationFunction.java:112,147,196), so among
                                      docs of equal winning time the greatest docId wins. The reference merges segments in
                                      a thread-dependent order (:223), so its ties across segments are unspecified; here:
                                      among equal winning times the greatest (segment bind index, docId) wins. The
                                      accumulator knows nothing of a value column: any column is read at the winning row
                                      by pa_query_fetch_time_rows, so LASTWITHTIME(a, ts, ..) and LASTWITHTIME(b, ts, ..)
                                      share one aggregation. A dictionary time column: num_values = size of its table-wide
                                      dictionary, ids in value order, segment dictIds mapped by pa_query_bind_value_remap.
                                      The scan keeps per group the maximum of one 64-bit word, time key << row bits |
                                      (segment << doc bits | doc) + 1 (0 = no row; "packed", one launch), or — a raw time
                                      column whose range does not fit beside the row — the maximum time in one launch and
                                      the maximum row among the docs holding it in a second ("wide"):
                                      pa_query_time_row_form. pa_query_prepare fails with PA_EUNSUPPORTED over a hashed
                                      key space (so over raw group-by columns and expression keys), for a multi-value
                                      group-by or aggregation column in the query, for a time column that is multi-value,
                                      not INT / LONG, or dictionary-encoded in some bound segments only, next to
                                      aggregation filters or expressions, and where numGroupsLimit trimming would run in
                                      its first-position + sort form (the prefix walk admits these updates like any
                                      other). pa_query_fetch writes nothing for it */
#define PA_AGG_FIRST_ROW_BY_TIME 9 /* FIRSTWITHTIME: the same with the smallest time (a doc with time <= the best takes
                                      over, FirstWithTimeAggregationFunction.java:111,147,200: among equal winning times
                                      again the greatest (segment bind index, docId) wins); the time key is complemented
                                      inside its width */
#define PA_AGG_MOMENTS 10 /* VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP of column `column_id`, or — with a second
                             column named through pa_query_set_moments — COVAR_POP / COVAR_SAMP of the pair: per group
                             the moment sums all of these finish from, so the spellings over one column (pair) share one
                             aggregation. Integer form (every argument column INT / LONG with all values inside int32 in
                             every bound segment): exact integers — sum x in one int64, sum x^2 (covariance: sum x, sum y,
                             sum x y) with the product as the 96-bit pair of PA_ACC_SUM_I64X2 — so the result does not
                             depend on the order of the atomics. Double form (everything else): variance keeps sum d and
                             sum d^2 of d = x - pivot in double, pivot = the midpoint of the column's minimum and maximum
                             over the bound segments (0 where that is not finite); covariance keeps the reference's raw
                             sums of x, y and x y in double. Without pa_query_set_moments every PA_AGG_MOMENTS is a
                             variance and the library chooses form and pivot (pa_query_moments_form reports them).
                             pa_query_prepare fails with PA_EUNSUPPORTED over a hashed key space (so over raw group-by
                             columns and expression keys), for a multi-value group-by or aggregation column in the query,
                             for an argument column that is multi-value, STRING or BYTES, next to aggregation filters or
                             expressions, and where numGroupsLimit trimming would run in its first-position + sort form
                             (the prefix walk admits these updates like any other). pa_query_fetch writes nothing for it:
                             pa_query_fetch_moments reads the tuples */
/* SUM / MIN / MAX / DISTINCTCOUNTHLL over a multi-value column aggregate every value of the doc (SUMMV, MINMV, MAXMV,
 * DISTINCTCOUNTHLLMV); a multi-value group-by column expands a doc into one key per value (cartesian product over
 * several MV columns), as DictionaryBasedGroupKeyGenerator.getIntRawKeys does. */

/* ---------------------------------------------------------------- device / errors */
int pa_abi_version(void);
int pa_device_count(void);
int pa_set_device(int device);
const char* pa_last_error(void);
/* Page-locked host memory of the library's runtime, for fetch output arrays: pa_query_fetch then copies each result
 * column straight into it by DMA (a pooled buffer the caller reuses across fetches). NULL on failure. */
void* pa_host_alloc(uint64_t bytes);
void pa_host_free(void* p);

/* ---------------------------------------------------------------- segments (HBM resident) */
typedef struct pa_segment pa_segment;

pa_segment* pa_segment_create(int32_t num_docs);

/* fwd_index: FixedBitSVForwardIndexWriter bytes, length must equal ceil(num_docs*num_bits/8)
 * (FixedBitIntReaderWriter.java:31 precondition). dict_values: int64[cardinality] for INT/LONG,
 * double[cardinality] for FLOAT/DOUBLE, NULL for STRING/BYTES. dict_hashes (nullable): MurmurHash
 * (stream-lib 2.9.8 MurmurHash.hash(Object)) of every dictionary value, required only to run
 * DISTINCTCOUNTHLL on STRING/BYTES dictionaries (numeric ones are hashed on the GPU). */
int pa_segment_add_sv_dict_column(pa_segment* seg, int32_t column_id, const uint8_t* fwd_index,
                                  uint64_t fwd_index_bytes, int32_t num_bits_per_value,
                                  int32_t cardinality, int32_t value_type, const void* dict_values,
                                  const int32_t* dict_hashes);

/* fwd_index: FixedBitMVForwardIndexReader layout (chunk offsets | row-start bitmap | bit-packed values). */
int pa_segment_add_mv_dict_column(pa_segment* seg, int32_t column_id, const uint8_t* fwd_index,
                                  uint64_t fwd_index_bytes, int32_t num_bits_per_value,
                                  int32_t cardinality, int64_t total_num_values, int32_t value_type,
                                  const void* dict_values, const int32_t* dict_hashes);

/* values: int32[num_docs] (INT), int64 (LONG), float (FLOAT), double (DOUBLE). */
int pa_segment_add_raw_column(pa_segment* seg, int32_t column_id, int32_t value_type,
                              const void* values);

int32_t pa_segment_num_docs(const pa_segment* seg);
uint64_t pa_segment_device_bytes(const pa_segment* seg);
void pa_segment_destroy(pa_segment* seg);

/* ---------------------------------------------------------------- query shape */
typedef struct {
  int32_t column_id;
  int32_t kind; /* PA_LEAF_* */
} pa_leaf_spec;

typedef struct {
  int32_t type;      /* PA_AGG_* */
  int32_t column_id; /* ignored for COUNT */
  int32_t log2m;     /* DISTINCTCOUNTHLL only (CommonConstants.Helix.DEFAULT_HYPERLOGLOG_LOG2M = 8) */
  int32_t flags;     /* PA_AGGF_* */
  int64_t num_values; /* DISTINCTCOUNT / VALUE_HISTOGRAM, and LAST / FIRST_ROW_BY_TIME over a dictionary time column: size
                         of the column's table-wide value dictionary (ignored otherwise) */
} pa_agg_spec;

/* SUM over an INT/LONG column: keep the exact 96-bit (low 32 unsigned, high 32 signed) pair accumulator
 * (PA_ACC_SUM_I64X2) even when every value of the bound segments fits int32. A multi-GPU query sets it on every rank
 * when any rank holds a value outside int32, so all ranks get the same accumulator layout for the RCCL reduce. */
#define PA_AGGF_WIDE_SUM 1

typedef struct {
  int32_t num_leaves;
  pa_leaf_spec leaves[PA_MAX_LEAVES];
  int32_t num_ops; /* 0 = match all (MatchAllFilterOperator) */
  int32_t ops[PA_MAX_OPS];
  int32_t num_group_by; /* 0 = aggregation-only query */
  int32_t group_by_columns[PA_MAX_GROUP_BY];
  int64_t group_by_cardinality[PA_MAX_GROUP_BY]; /* size of the table-wide key space per column; 0 for a raw
                                                     (no-dictionary) column, grouped by value
                                                     (NoDictionarySingle/MultiColumnGroupKeyGenerator) */
  int32_t num_aggs;
  pa_agg_spec aggs[PA_MAX_AGGS];
  int32_t flags; /* PA_QF_* */
  int32_t num_groups_limit; /* numGroupsLimit (QueryOptionsUtils / InstancePlanMakerImplV2, default 100000); 0 = none.
                               When some segment can hold that many distinct groups, the reference's first-seen trimming
                               runs on the GPU (DictionaryBasedGroupKeyGenerator IntGroupIdMap.getGroupId :992-1017) */
  int64_t hash_keys_bound; /* hashed key spaces: the table holds at least 2 x this many keys (0 = size from the bound
                              segments alone). A multi-GPU query passes the largest per-rank bound of all ranks so every
                              rank's table can hold its share of the cross-GPU merge (parallel.table_layout) */
  int32_t flags2; /* PA_QF2_* */
  int32_t reserved2;
} pa_query_spec;

#define PA_QF_STAGE_ALL 1  /* stage post-filter columns through LDS even when a filter exists */
#define PA_QF_FORCE_GLOBAL 2 /* force global-memory accumulators (testing the fallback) */
/* tuning overrides of the tile planner (0 = automatic) */
#define PA_QF_STEPS16 (1 << 4)        /* 1024-doc wave tiles */
#define PA_QF_STEPS32 (1 << 5)        /* 2048-doc wave tiles */
#define PA_QF_NO_LAZY (1 << 6)        /* evaluate every filter clause on staged tiles (no late materialisation) */
#define PA_QF_FORCE_LDS (1 << 7)      /* LDS-privatised accumulators even for sparse results (when they fit) */
#define PA_QF_RING_SHIFT 8            /* bits 8..11: tile images per wave (2..8) */
#define PA_QF_WG_SHIFT 12             /* bits 12..14: workgroups per CU (1..4) */
#define PA_QF_NO_GDENSE_LM (1 << 15)      /* dense GROUP BY kernel: the step-major walk (ds_read2 per doc and column) instead
                                             of the lane-major one (each lane unpacks its 16 docs of every column) */
#define PA_QF_NO_JIT (1u << 31)          /* never the query-shape specialised dense kernel (gdl_jit.hip) */
#define PA_QF_GD_DRAIN_EACH_TILE (1 << 2) /* testing: packed dense accumulation drains each wave's rows after every tile */
#define PA_QF_NO_GD_PACK (1 << 3)         /* dense GROUP BY, lane-major walk: one LDS atomic per aggregation and matching doc
                                             instead of one packed word (COUNT + SUM terms) per matching doc */
#define PA_QF_DEBUG_STREAM_ONLY (1 << 16) /* measurement only: stream the tiles, skip decode (results invalid) */
#define PA_QF_NO_LANE_MAJOR (1 << 17)     /* use the step-major scan kernel even when the lane-major one applies */
#define PA_QF_NO_REG_STAGE (1 << 18)      /* dense GROUP BY kernel: tiles staged by the LDS-DMA ring only, never through
                                             VGPRs (the register-staged variants keep more bytes in flight beside large
                                             LDS tables) */
#define PA_QF_NO_BOX_FILTER (1 << 19)     /* dense GROUP BY kernel: evaluate the filter even when it is exactly the group-key
                                             box (unit range clauses on group-by columns), then walk the matching docs */
#define PA_QF_BOX_FILTER (1 << 20)        /* dense GROUP BY kernel: take the key box as the filter (every doc box-checked
                                             instead of filter + walk) when it is exactly the filter; opt-in */
#define PA_QF_NO_PARTITION (1 << 21)      /* high-cardinality dense GROUP BY: per-doc global atomics, not partitioned */
#define PA_QF_NO_SPLIT_EMIT (1 << 24)     /* partitioned aggregation with both record streams: one emit kernel for both
                                             (default: a V launch and an H launch, each holding only its own bins) */
#define PA_QF_NO_LIMIT_WALK (1 << 25)     /* numGroupsLimit: first-position + sort trimming even where the prefix walk applies */
#define PA_QF_NO_LANE_ACC (1 << 26)       /* aggregation-only query: LDS/global accumulators instead of per-lane registers */
#define PA_QF_NO_LANE_HIST (1 << 27)      /* aggregation-only SUM over a shared dictionary: gather each doc's value instead
                                             of counting dictIds in an LDS histogram */
#define PA_QF_LAZY_POST (1 << 28)         /* post-filter columns (group-by keys, aggregated values) read per matching doc
                                             from HBM at any filter density, never staged with the filter columns */
#define PA_QF_NO_DENSE_GROUP (1 << 29)    /* filter + GROUP BY over a small key space: the LDS strategy (post-filter
                                             columns per matching doc from HBM) instead of the dense group-by kernel
                                             (every column staged, value dictionaries and remaps in LDS) */
#define PA_QF_NO_FILTER_STATS (1 << 30)   /* the scan does NOT count what the execution statistics of an AND of two scan
                                             leaves need (by default it does wherever that fused count applies:
                                             pa_query_leap_leaf / pa_query_leap_counts / pa_query_execution_stats) */
#define PA_QF2_NO_COUNT_FREE 1         /* partitioned plans: the count + emit passes even where the count-free emit
                                           (pve_jit.hip, pa_query_count_free_emit) applies */
#define PA_QF_PART_SHIFT 22              /* bits 22..23: LDS per partition of the partitioned aggregation (0 = auto,
                                             1 = 64 KiB, 2 = 96 KiB, 3 = 144 KiB): larger partitions = fewer record
                                             write fronts per XCD */

/* per-(segment, leaf) parameters in that segment's dictId space */
typedef struct {
  int32_t lo, hi;       /* DICT_RANGE: lo <= dictId < hi */
  int32_t negate;       /* result XOR negate */
  int32_t reserved;
  const uint32_t* lut;  /* DICT_SET: host bitmap, ceil(cardinality/32) words, bit (id&31) of word id>>5 */
  int64_t ilo, ihi;     /* RAW_RANGE on INT/LONG, inclusive */
  double dlo, dhi;      /* RAW_RANGE on FLOAT/DOUBLE, inclusive */
  const void* values;   /* RAW_SET: host int64_t[num_values] (INT/LONG column) or double[num_values] (FLOAT/DOUBLE:
                           the stored float widened), strictly ascending; copied at bind */
  int64_t num_values;
} pa_leaf_params;

typedef struct pa_query pa_query;

pa_query* pa_query_create(const pa_query_spec* spec, int32_t num_segments);

/* group_remaps[j]: host int32[segment cardinality of group_by_columns[j]] mapping the segment's dictId
 * to the table-wide key id of that column (NULL = identity). */
int pa_query_bind_segment(pa_query* q, int32_t index, const pa_segment* seg,
                          const pa_leaf_params* leaf_params, const int32_t* const* group_remaps);

/* DISTINCTCOUNT or VALUE_HISTOGRAM aggregation `agg` on the segment bound at `index`: remap[d] = the table-wide value id of the segment's
 * dictId d (int32[segment cardinality]; NULL = identity, the segment's dictionary IS the table-wide one). Call after
 * pa_query_bind_segment, before pa_query_prepare. Also a LAST / FIRST_ROW_BY_TIME aggregation whose time column is
 * dictionary-encoded in that segment: the table-wide ids must follow the order of the values (PA_EINVAL for a raw time
 * column, whose values the scan reads directly). */
int pa_query_bind_value_remap(pa_query* q, int32_t index, int32_t agg, const int32_t* remap);

/* ---------------------------------------------------------------- selection queries
 * SELECT columns ... [WHERE filter] [ORDER BY c1 [DESC], ...] LIMIT [offset,] n. The query is created from an
 * aggregation-only spec (its filter is the selection's; its aggregations are ignored, e.g. one COUNT) and turned into
 * a selection before any segment is bound. The result is the num_rows smallest matching docs of all bound segments
 * under the ORDER BY comparator (SelectionOrderByOperator.java:108-112), ties broken by (segment bind index, docId)
 * ascending; without ORDER BY the first num_rows matching docs in that order (SelectionOnlyOperator.java).
 *
 * Sort key: one unsigned 64-bit word, the ORDER BY components most significant first. A dictionary column contributes
 * its table-wide value id (ceil(log2(cardinality)) bits; 0 bits for a dictionary of one value) through a per-segment
 * remap, so ids must follow the order of the values (STRING: String.compareTo, i.e. UTF-16 code units). A raw INT /
 * LONG column contributes the value with its sign bit flipped (32 / 64 bits), a raw FLOAT / DOUBLE column the
 * total-order image of the value with every NaN made the canonical one first (Double.compare: -0.0 < 0.0, NaN
 * greatest). A descending component is complemented inside its width. pa_query_prepare fails with PA_EUNSUPPORTED for
 * components wider than 64 bits together, for multi-value or BYTES columns, and for a column that is
 * dictionary-encoded in some bound segments only. */
typedef struct {
  int32_t num_order_by;
  int32_t order_by_columns[PA_MAX_ORDER_BY];
  int32_t order_by_desc[PA_MAX_ORDER_BY];          /* 1 = descending */
  int64_t order_by_cardinality[PA_MAX_ORDER_BY];   /* size of the column's table-wide dictionary; 0 = a raw column,
                                                      ordered by value */
  int32_t num_columns;
  int32_t columns[PA_MAX_SELECT_COLUMNS];          /* output columns (pa_query_fetch_selection's out_cells order) */
  int32_t num_rows;                                /* offset + limit (SelectionOrderByOperator._numRowsToKeep),
                                                      1..PA_MAX_SELECT_ROWS, else PA_EUNSUPPORTED */
} pa_select_spec;

/* Before pa_query_bind_segment and pa_query_prepare. pa_query_execute / reset / scan then drive the selection's scan;
 * pa_query_fetch fails on such a query (pa_query_fetch_selection reads it); pa_query_matched_docs, the leaf bitmaps
 * and pa_query_execution_stats work as for an aggregation. */
int pa_query_set_selection(pa_query* q, const pa_select_spec* spec);

/* remap[d] = the table-wide value id of dictId d of ORDER BY column `order_by_index` in the segment bound at
 * `segment_index` (int32[segment cardinality], every id < order_by_cardinality; NULL = identity): the role
 * pa_query_bind_segment's group_remaps play for GROUP BY. After pa_query_bind_segment, before pa_query_prepare. */
int pa_query_bind_order_remap(pa_query* q, int32_t segment_index, int32_t order_by_index, const int32_t* remap);

/* The result of the last scan: min(num_rows, matched docs) rows in ascending (key, segment, doc) order; row r is doc
 * out_docs[r] of the segment bound at out_segments[r] with sort key out_keys[r] (each array holds `capacity` elements;
 * any may be NULL). out_cells[c] (int64[capacity], may be NULL) takes output column c of every row: the segment's
 * dictId for a dictionary column (the host decodes it through that segment's dictionary, as
 * SelectionOperatorUtils.getRowsFromBlock does through the block's value sets), the value of a raw INT / LONG column,
 * the bits of the value as a double for a raw FLOAT / DOUBLE column. Returns the number of rows (may exceed capacity:
 * then only `capacity` were written), <0 on error; capacity = 0 only counts. Replaces the queue drain of
 * SelectionOrderByOperator.java:193-322 and SelectionOrderByCombineOperator's merge. Synchronises `stream`. */
int64_t pa_query_fetch_selection(pa_query* q, void* stream, int64_t capacity, int32_t* out_segments, int32_t* out_docs,
                                 uint64_t* out_keys, int64_t* const* out_cells);

/* Docs of every bound segment that passed the filter in the scan the last pa_query_fetch_selection read
 * (int64[num_segments]): SelectionOrderByOperator's per-segment numDocsScanned, which its numEntriesScannedPostFilter
 * needs (SelectionOrderByOperator.java:175,239,300). */
int pa_query_selection_segment_docs(const pa_query* q, int64_t* out);

/* Counters of that scan, for tests and measurement: out[0] = candidates the scan waves appended, out[1] = in-place
 * compactions they ran (a wave's candidate segment filled), out[2] = scan waves launched, out[3] = candidates per wave
 * (CAP). */
int pa_query_selection_counters(const pa_query* q, int64_t* out);

/* ---------------------------------------------------------------- distinct queries
 * SELECT DISTINCT c1, c2, ... [WHERE filter] [ORDER BY ci [DESC], ...] [LIMIT n] (DistinctOperator +
 * DistinctCombineOperator). The query is created from a GROUP BY spec without aggregations (num_aggs = 0): its group-by
 * columns are the DISTINCT columns, with cardinalities and per-segment remaps bound as for GROUP BY, and it is turned
 * into a distinct query before pa_query_prepare. The scan sets one bit per key of the direct key space
 * (sum_j id_j * prod_{k<j} card_k) in the PA_ACC_KEYBITS_U32 section; the finish orders the present keys.
 *
 * Order: the ORDER BY entries first (each an index into the group-by columns, ascending or descending by table-wide
 * value id), then every DISTINCT column not named, ascending, in select order: a total order of the keys, so the rows
 * a limit keeps are a function of the data. Table-wide ids must therefore follow the order of the values.
 *
 * pa_query_prepare fails with PA_EUNSUPPORTED for raw (no-dictionary), multi-value and BYTES columns, for a key space
 * of more than 2^31 keys, and for ORDER BY with limit > PA_MAX_SELECT_ROWS over a key space larger than that (a limit
 * of the interface: the finish itself has no such bound). Without ORDER BY any limit >= 0 is accepted.
 * When the order is not the key's own digit order (any ORDER BY but the single column ascending; two or more columns
 * without ORDER BY) pa_query_prepare allocates a second bitmap of the key space's size (up to 256 MiB), which every
 * fetch clears and fills. */
typedef struct {
  int32_t num_order_by;
  int32_t order_by_index[PA_MAX_GROUP_BY];  /* index into the spec's group-by columns; each at most once */
  int32_t order_by_desc[PA_MAX_GROUP_BY];   /* 1 = descending */
  int64_t limit;
} pa_distinct_spec;

/* Before pa_query_prepare. pa_query_execute / reset / scan then drive the distinct scan; pa_query_fetch fails with
 * PA_EINVAL on such a query (pa_query_fetch_distinct reads it, and like pa_query_fetch fails with PA_EINVAL while a
 * tuning that skips work is set). */
int pa_query_set_distinct(pa_query* q, const pa_distinct_spec* spec);

/* The result of the last scan: min(limit, keys present) rows in final order, row-major in out_ids (int32[capacity *
 * num_group_by]): one table-wide value id per DISTINCT column. *out_present (may be NULL) = distinct keys present,
 * before the limit. Returns the number of rows (may exceed capacity: then only `capacity` were written), <0 on error;
 * capacity = 0 only counts. Synchronises `stream`. */
int64_t pa_query_fetch_distinct(pa_query* q, void* stream, int64_t capacity, int32_t* out_ids, int64_t* out_present);

/* ---------------------------------------------------------------- filtered aggregations
 * AGG(col) FILTER (WHERE f) (AggregationFunctionUtils.buildFilteredAggregationInfos :312-396,
 * FilteredAggregationOperator.java:66-101, FilteredGroupByOperator.java:107-200). Aggregations with an equal filter
 * share a lane; the ones without a filter form the main lane; lane j aggregates the docs matching W AND F_j, where W is
 * the spec's filter. One fused scan streams the columns once and applies every lane's filter to the docs W kept.
 *
 * The filters' leaves are appended to pa_query_spec.leaves after the main filter's (inside PA_MAX_LEAVES), so
 * pa_query_bind_segment's pa_leaf_params bind them like any other leaf; spec.ops holds only the main filter's program.
 * spec.aggs may then hold the same (type, column) several times under different filters, and several PA_AGG_COUNT
 * entries (a filtered COUNT is its lane's doc count: pa_query_fetch_lane_counts; pa_query_fetch writes the group's
 * count for every PA_AGG_COUNT).
 *
 * A group exists when any lane saw a doc of it (the shared group-key generator, FilteredGroupByOperator.java:117-150):
 * PA_ACC_COUNT_U64 counts the docs of the union of the lanes, which is W when some aggregation has no filter.
 * Accumulators of a lane that saw no doc of a group stay at their reset identities; the lane count tells (MIN / MAX of
 * such a cell are not meaningful in pa_query_fetch's output).
 *
 * pa_query_prepare fails with PA_EUNSUPPORTED for a hashed key space, for multi-value columns anywhere but a leaf of the
 * main filter, for PA_AGG_VALUE_HISTOGRAM / PA_AGG_COUNT_MV under a filtered query, and when numGroupsLimit trimming
 * would run (the reference's first-seen order is lane-major). */
typedef struct {
  int32_t num_filters;                        /* 1..PA_MAX_AGG_FILTERS */
  int32_t num_ops[PA_MAX_AGG_FILTERS];        /* >= 1 */
  int32_t ops[PA_MAX_AGG_FILTERS][PA_MAX_OPS]; /* postfix programs (PA_OP_*) over pa_query_spec.leaves */
  int32_t agg_filter[PA_MAX_AGGS];            /* per spec.aggs[i]: its filter, or -1 (the main lane) */
} pa_agg_filter_spec;

/* Between pa_query_create and the first pa_query_bind_segment. PA_EINVAL: counts out of range, a malformed program, a
 * filter no aggregation uses; PA_EUNSUPPORTED: a filter expanding to more than PA_MAX_LEAVES CNF literals. */
int pa_query_set_agg_filters(pa_query* q, const pa_agg_filter_spec* spec);

/* ---------------------------------------------------------------- moments (PA_AGG_MOMENTS)
 * What pa_agg_spec has no room for, per spec.aggs[i] (entries of other aggregation types are ignored). */
#define PA_MOMENTS_FORM_AUTO 0    /* the library chooses: integer where every argument column allows it */
#define PA_MOMENTS_FORM_INTEGER 1 /* exact integer sums (PA_ACC_MOM_I64); PA_EINVAL at prepare where a column does not
                                     fit */
#define PA_MOMENTS_FORM_DOUBLE 2  /* double sums (PA_ACC_MOM_F64) */
typedef struct {
  int32_t second_column[PA_MAX_AGGS]; /* -1: variance of column_id; else covariance of (column_id, second_column) */
  int32_t form[PA_MAX_AGGS];          /* PA_MOMENTS_FORM_* (ranks of a multi-GPU query pass the agreed form) */
  int32_t has_pivot[PA_MAX_AGGS];     /* 1: `pivot` is the variance's pivot in the double form (ranks pass the agreed
                                         value); 0: the library takes the midpoint of the bound segments' min and max */
  double pivot[PA_MAX_AGGS];          /* must be finite */
} pa_moments_spec;

/* Between pa_query_create and pa_query_prepare. PA_EINVAL: a form outside PA_MOMENTS_FORM_*, a pivot that is not finite,
 * a pivot on a covariance. */
int pa_query_set_moments(pa_query* q, const pa_moments_spec* spec);

/* The form (PA_MOMENTS_FORM_INTEGER / _DOUBLE) and pivot the prepared query uses for aggregation `agg` (either pointer
 * may be NULL; the pivot of the integer form and of a covariance is 0). PA_EINVAL: not prepared, or not a PA_AGG_MOMENTS. */
int pa_query_moments_form(const pa_query* q, int32_t agg, int32_t* out_form, double* out_pivot);

/* Docs of every lane in the groups the last pa_query_fetch returned, in the same order (num_groups = that call's
 * result): out[j * num_groups + g] (int64[num_filters * num_groups]) = docs of group g matching W AND F_j. The host
 * reads COUNT and AVG of a filtered aggregation from it. Synchronises `stream`. */
int pa_query_fetch_lane_counts(pa_query* q, void* stream, int64_t num_groups, int64_t* out);

/* Per bound segment s of the last scan: out[s * (num_filters + 1)] = docs matching W, out[s * (num_filters + 1) + 1 + j]
 * = docs matching W AND F_j (int64[num_segments * (num_filters + 1)]): what numDocsScanned and
 * numEntriesScannedPostFilter of a filtered query are summed from (FilteredAggregationOperator.java:96-98,
 * FilteredGroupByOperator.java:159-161), with each segment's own lane structure. After a pa_query_fetch of that scan it
 * returns the counters that fetch read with its own copy (no synchronisation); else it synchronises the device. */
int pa_query_lane_docs(pa_query* q, int64_t* out);

/* ---------------------------------------------------------------- transform expressions
 * SUM(ADD(a, b)), AVG(SUB(a, b)), GROUP BY timeConvert(ts, 'MILLISECONDS', 'DAYS'), ...: the TransformOperator the
 * reference's AggregationPlanNode / GroupByPlanNode put between projection and executor (operator/transform/function/
 * AdditionTransformFunction, SubtractionTransformFunction, MultiplicationTransformFunction, DivisionTransformFunction,
 * ModuloTransformFunction, SingleParamMathTransformFunction (abs / ceil / floor), TimeConversionTransformFunction), whose
 * block values the aggregation functions and NoDictionary{Single,Multi}ColumnGroupKeyGenerator read. Here every
 * expression is a short three-address program the scan runs per matching doc, after one gather of the operand columns.
 *
 * An operation is dst = op(a, b) over PA_MAX_EXPR_REGS value registers, each holding a double (D) or an int64 (L).
 * An operand is a register (PA_EXPR_ARG_REG, a = its index), an immediate double (PA_EXPR_ARG_F64, imm = its bits) or an
 * immediate int64 (PA_EXPR_ARG_I64, imm = the value); LOAD_COL alone names a column (PA_EXPR_ARG_COL, a = index into
 * pa_expr_spec.columns) and takes the conversion in b (PA_EXPR_DOUBLE / PA_EXPR_LONG: the reference's
 * transformToDoubleValuesSV / transformToLongValuesSV of an INT / LONG / FLOAT / DOUBLE column, dictionary-encoded or
 * raw: (double)value resp. the Java (long) cast).
 *   LOAD_COL            D or L
 *   ADD SUB MUL DIV MOD D x D -> D  (IEEE double; MOD is Java's % = C fmod; a register or a double immediate each)
 *   ABS CEIL FLOOR      D -> D
 *   D2L                 D -> L      (Java (long): NaN -> 0, saturating)
 *   L2D                 L -> D
 *   TCONV_DIV           L / imm     (b: int64 immediate > 0; truncating toward zero: TimeUnit.convert to a coarser unit)
 *   TCONV_MUL           L * imm     (b: int64 immediate > 0; saturating at Long.MIN_VALUE / MAX_VALUE: to a finer unit)
 * The program's value is the register its last operation wrote; its type must be result_type.
 *
 * An aggregation (SUM / MIN / MAX only) with agg_expr[i] >= 0 aggregates that program's value in place of a column: a
 * double value as a DOUBLE column's (PA_ACC_SUM_F64; MIN / MAX in the ordered encoding), an int64 value as a LONG
 * column's (the exact PA_ACC_SUM_I64X2 pair). A group-by position with group_by_expr[j] >= 0 groups by the value's 64
 * bits (every NaN made 0x7ff8000000000000 first; -0.0 and 0.0 stay distinct: Double.doubleToLongBits, the hash the
 * reference's Double2IntOpenHashMap uses) exactly as a raw LONG / DOUBLE column's component: the key space is hashed,
 * pa_query_key_layout reports the component's shift, and group_by_cardinality[j] is ignored. The spec's column_id at
 * those positions is ignored.
 *
 * A query with expressions runs one of two strategies of its own (workgroup-private LDS accumulators over a direct key
 * space, or device-scope atomics). pa_query_prepare fails with PA_EUNSUPPORTED when numGroupsLimit trimming would run,
 * for multi-value, STRING or BYTES operand columns, and next to aggregation filters. */
#define PA_EXPR_DOUBLE 0
#define PA_EXPR_LONG 1

#define PA_EXPR_ARG_REG 0
#define PA_EXPR_ARG_COL 1
#define PA_EXPR_ARG_F64 2
#define PA_EXPR_ARG_I64 3

#define PA_EXPR_LOAD_COL 0
#define PA_EXPR_ADD 1
#define PA_EXPR_SUB 2
#define PA_EXPR_MUL 3
#define PA_EXPR_DIV 4
#define PA_EXPR_MOD 5
#define PA_EXPR_ABS 6
#define PA_EXPR_CEIL 7
#define PA_EXPR_FLOOR 8
#define PA_EXPR_D2L 9
#define PA_EXPR_L2D 10
#define PA_EXPR_TCONV_DIV 11
#define PA_EXPR_TCONV_MUL 12

typedef struct {
  int32_t op;     /* PA_EXPR_* opcode */
  int32_t dst;    /* 0..PA_MAX_EXPR_REGS-1 */
  int32_t a_kind; /* PA_EXPR_ARG_* */
  int32_t a;      /* register / column index */
  int32_t b_kind;
  int32_t b;      /* register index; LOAD_COL: PA_EXPR_DOUBLE / PA_EXPR_LONG */
  int64_t a_imm;  /* immediate: the double's bits, or the int64 */
  int64_t b_imm;
} pa_expr_op;

typedef struct {
  int32_t result_type; /* PA_EXPR_DOUBLE / PA_EXPR_LONG */
  int32_t num_ops;     /* 1..PA_MAX_EXPR_OPS */
  pa_expr_op ops[PA_MAX_EXPR_OPS];
} pa_expr_program;

typedef struct {
  int32_t num_exprs;   /* 1..PA_MAX_EXPRS */
  int32_t num_columns; /* 1..PA_MAX_EXPR_COLUMNS */
  int32_t columns[PA_MAX_EXPR_COLUMNS];     /* column ids of the distinct operand columns */
  int32_t agg_expr[PA_MAX_AGGS];            /* per spec.aggs[i]: its expression, or -1 */
  int32_t group_by_expr[PA_MAX_GROUP_BY];   /* per group-by position: its expression, or -1 */
  pa_expr_program exprs[PA_MAX_EXPRS];
} pa_expr_spec;

/* Between pa_query_create and the first pa_query_bind_segment (a bind reads the spec's columns, which this call
 * replaces at the expressions' positions). PA_EINVAL: a call after a bind, counts out of range, an index outside its table, a register
 * read before it was written, an operand of the wrong type, an expression no aggregation or group-by position uses or
 * that reads no column, an expression under an aggregation other than SUM / MIN / MAX, a selection or distinct query;
 * PA_EUNSUPPORTED: a query with aggregation filters. */
int pa_query_set_expressions(pa_query* q, const pa_expr_spec* spec);

/* Tests and measurement only: overrides one planner decision of this query (the tunings, their ranges and defaults:
 * pinot_amd/csrc/pa_tuning.h; the library reads none of them from the environment). Before pa_query_prepare.
 * PA_EINVAL: unknown name, value outside the tuning's range, or query already prepared. */
int pa_query_set_tuning(pa_query* q, const char* name, int32_t value);
/* 1 when a tuning that skips work is set (results invalid: pa_query_fetch, pa_query_pack_rows and pa_query_merge_rows
 * then fail; execute and scan still run, for timing), else 0; -1 for a null query. */
int32_t pa_query_results_invalid(const pa_query* q);

/* Uploads per-segment parameters, builds the tile schedule and HLL lookup tables, sizes the
 * accumulators. Must be called once after every segment is bound. */
int pa_query_prepare(pa_query* q);

/* Number of keys of the table-wide key space (1 for aggregation-only queries). */
int64_t pa_query_num_keys(const pa_query* q);

/* Zeroes the accumulators and runs the fused scan (filter + group-key + aggregate) over every bound
 * segment on `stream` (hipStream_t, NULL = default stream). Asynchronous. Equivalent to pa_query_reset followed by
 * pa_query_scan (the two halves exist so a caller can time the scan kernel alone). */
int pa_query_execute(pa_query* q, void* stream);
int pa_query_reset(pa_query* q, void* stream);
int pa_query_scan(pa_query* q, void* stream);

/* Accumulator sections, for the cross-GPU RCCL reduce. section kinds: */
#define PA_ACC_COUNT_U64 0 /* reduce SUM */
#define PA_ACC_SUM_I64 1   /* reduce SUM */
#define PA_ACC_SUM_F64 2   /* reduce SUM */
#define PA_ACC_MIN_I64 3   /* reduce MIN (ordered encoding for floating values) */
#define PA_ACC_MAX_I64 4   /* reduce MAX */
#define PA_ACC_HLL_U8 5    /* reduce MAX; one byte per register: [key << log2m | register] */
#define PA_ACC_SUM_I64X2 6 /* reduce SUM; [2k] = sum of low 32 bits (unsigned), [2k+1] = sum of high 32 bits */
#define PA_ACC_DOCS_U64 7  /* reduce SUM; [0] docs that passed the filter (numDocsScanned), [1] group-table overflows,
                              [2] segments whose distinct groups reached numGroupsLimit, [3] internal consistency
                              errors (must stay 0; fetch fails otherwise) */
#define PA_ACC_KEYS_I64 8  /* hashed key space only: slot -> packed key (INT64_MAX = empty); not element-wise
                              reducible across GPUs (slots differ): merge fetched groups by key instead */
#define PA_ACC_PRESENCE_U8 9 /* reduce MAX; DISTINCTCOUNT: [key * stride + value id] = 1 if the group saw the value,
                                stride = num_values rounded up to 16 bytes */
#define PA_ACC_HIST_U64 10 /* reduce SUM; VALUE_HISTOGRAM: [key * stride + value id] = times the group aggregated the
                              value, stride = num_values rounded up to a multiple of 2 (whole 16-byte units; a padding
                              bin stays 0). 64 bits: a GPU holds tens of billions of docs, so one bin can pass 2^32 */
#define PA_ACC_KEYBITS_U32 11 /* reduce bitwise OR; distinct queries: bit (key & 31) of word (key >> 5) = the key is
                                 present; the only per-key section of such a query (reset identity 0) */
#define PA_ACC_LANE_COUNT_U64 12 /* reduce SUM; filtered aggregations: [lane * num_keys + key] = docs of that lane (W AND
                                    F_lane) in that group (reset identity 0) */
#define PA_ACC_TIME_ROW_U64 13 /* LAST / FIRST_ROW_BY_TIME: [key] = the group's winning word (packed form: time key <<
                                  row bits | row + 1; wide form: row + 1), reset identity 0 = no row. Not element-wise
                                  reducible across GPUs: the segment index in the row is rank-local, and the row's values
                                  live on the rank that holds it */
#define PA_ACC_TIME_MAX_I64 14 /* the wide form's first word: [key] = the greatest time of the group's docs (FIRST: of
                                  the complemented times), reset identity INT64_MIN; read by the second scan launch */
/* PA_AGG_MOMENTS: PA_MOMENTS_WORDS = 4 64-bit words per key, [key * 4 + w], reset identity 0, reduce SUM (ranks must agree
 * on form and pivot). p = x * x for a variance, x * y for a covariance (the second column's value y):
 *   PA_ACC_MOM_I64  w0 = sum x (int64), w1 = sum y (covariance; else unused), w2 = sum of the low 32 bits of p
 *                   (unsigned), w3 = sum of p >> 32 (signed): sum p = w3 * 2^32 + w2, as PA_ACC_SUM_I64X2
 *   PA_ACC_MOM_F64  doubles: w0 = sum x' , w1 = sum y (covariance; else unused), w2 = sum x' * y', w3 unused; variance:
 *                   x' = y' = x - pivot, covariance: x' = x, y' = y */
#define PA_ACC_MOM_I64 15
#define PA_ACC_MOM_F64 16
#define PA_MOMENTS_WORDS 4
/* All sections live in one device block of pa_query_accumulator_bytes() bytes (256-byte aligned sections).
 * pa_query_set_accumulator_buffer lets the caller own that block (e.g. memory its collective library
 * registered) instead of the library: call after pa_query_prepare; `bytes` must be >= the size. */
uint64_t pa_query_accumulator_bytes(const pa_query* q);
int pa_query_set_accumulator_buffer(pa_query* q, void* device_buffer, uint64_t bytes);
int32_t pa_query_num_sections(const pa_query* q);
/* returns device pointer, writes kind and element count */
void* pa_query_section(const pa_query* q, int32_t section, int32_t* kind, int64_t* num_elements);

/* Compacts the non-empty keys (count > 0) in ascending key order and copies them to the host.
 * out_keys: int64[capacity]; out_counts: int64[capacity]; out_aggs[i]: double[capacity] for
 * COUNT/SUM/MIN/MAX (the reference's intermediate type), uint8[capacity << log2m] for HLL registers. Nothing is
 * written for a VALUE_HISTOGRAM aggregation (0 bytes per group: its out_aggs[i] may be NULL); its bins are read with
 * pa_query_fetch_histogram / pa_query_percentiles. Nor for a LAST / FIRST_ROW_BY_TIME aggregation (0 bytes per group):
 * pa_query_fetch_time_rows reads its rows; nor for a PA_AGG_MOMENTS aggregation: pa_query_fetch_moments reads its tuples.
 * For aggregation-only queries key 0 is always returned (count may be 0).
 * Returns the number of groups (may exceed capacity: then only `capacity` were written), <0 on error.
 * capacity = 0 (output pointers may be NULL) only counts the groups — for large key spaces just the GPU count pass —
 * so a caller can size its arrays exactly before the real fetch. Synchronises `stream`. */
int64_t pa_query_fetch(pa_query* q, void* stream, int64_t capacity, int64_t* out_keys,
                       int64_t* out_counts, void* const* out_aggs);

/* pa_query_fetch with the server's group trim done on the GPU: of the n non-empty groups only the `trim` smallest under
 * the ORDER BY comparator are gathered and copied, in ascending key order, into the same arrays as pa_query_fetch.
 * Replaces, for a direct key space, IndexedTable.finish (IndexedTable.java:149) with TableResizer.resizeRecordsMap
 * (TableResizer.java:187-238: the records' order-by values extracted, the top `trim` kept) at the capacity of
 * GroupByUtils.getTableCapacity / GroupByCombineOperator.java:63-73 (the caller passes it as `trim`: max(5 * limit,
 * minServerGroupTrimSize) under ORDER BY, else the limit).
 * A term compares a group-by column's value (PA_TRIM_KEY_COLUMN: by table-wide id — the table dictionaries are sorted
 * ascending), the group's count, or an aggregation's FINAL value as a double: a SUM / MIN / MAX exactly as pa_query_fetch
 * returns it (a 96-bit SUM rounded once, so sums that round to one double tie), AVG = that sum / count and MINMAXRANGE
 * = max - min in IEEE double; -0.0 ties with +0.0; `desc` reverses the term. Ties of all terms are broken by the group
 * key ids, group-by column 0 most significant, ascending. num_terms = 0 keeps the `trim` smallest key tuples. NaN term
 * values are out of scope: the comparator of the reference is no total order over them.
 * PA_EUNSUPPORTED (the caller trims the full fetch on the host instead): a hashed key space (so any expression key), a
 * query with a VALUE_HISTOGRAM, LAST / FIRST_ROW_BY_TIME or MOMENTS aggregation or aggregation filters (their fetch calls follow
 * the full fetch's group order), more than PA_MAX_TRIM_TERMS terms, a term over any other aggregation type (HLL, DISTINCTCOUNT, COUNT_MV).
 * HLL / DISTINCTCOUNT aggregations that are only read are gathered for the kept groups.
 * Returns min(n, trim) (may exceed capacity: then nothing was written; call again with that capacity), <0 on error;
 * *out_total_groups = n. With n <= trim the call is pa_query_fetch. Fills pa_query_matched_docs and
 * pa_query_num_groups_limit_reached as pa_query_fetch does. Synchronises `stream`. */
#define PA_TRIM_KEY_COLUMN 0   /* index = group-by position */
#define PA_TRIM_COUNT 1
#define PA_TRIM_AGG 2          /* index = aggregation (SUM / MIN / MAX): its final double */
#define PA_TRIM_AVG 3          /* index = SUM aggregation; value = sum / count */
#define PA_TRIM_RANGE 4        /* index = MAX aggregation, index2 = MIN aggregation */
#define PA_MAX_TRIM_TERMS 4
typedef struct {
  int32_t num_terms;
  int32_t kind[PA_MAX_TRIM_TERMS], index[PA_MAX_TRIM_TERMS], index2[PA_MAX_TRIM_TERMS], desc[PA_MAX_TRIM_TERMS];
  int64_t trim;
} pa_trim_spec;
int64_t pa_query_fetch_trimmed(pa_query* q, void* stream, const pa_trim_spec* spec, int64_t capacity,
                               int64_t* out_keys, int64_t* out_counts, void* const* out_aggs,
                               int64_t* out_total_groups);

/* The bins of VALUE_HISTOGRAM aggregation `agg` for the groups pa_query_fetch returns for the current accumulators, in
 * the same order (num_groups = that call's result): per group the non-zero bins in ascending table-wide value id, as
 * (value id, count) pairs. out_row_ends[g] (int64[num_groups]) = end offset of group g's pairs (its start is
 * out_row_ends[g - 1], 0 for g = 0); out_value_ids (int32[capacity]) / out_value_counts (int64[capacity]) hold the pairs.
 * Returns the total number of pairs (may exceed capacity: then only the first `capacity` pairs were written), <0 on
 * error. capacity = 0 only counts (the two pair arrays may be NULL). This is the intermediate result of
 * PercentileAggregationFunction.extractAggregationResult / extractGroupByResult (the DoubleArrayList of every value, as
 * value -> multiplicity) and of PercentileMVAggregationFunction; the non-zero count, scan and compaction run on the GPU
 * (pa_hist.hip), then one copy per output array. Synchronises `stream`. */
int64_t pa_query_fetch_histogram(pa_query* q, void* stream, int32_t agg, int64_t num_groups, int64_t capacity,
                                 int64_t* out_row_ends, int32_t* out_value_ids, int64_t* out_value_counts);

/* Final results of VALUE_HISTOGRAM aggregation `agg` for the same groups, without moving the bins: out_value_ids
 * [g * num_percentiles + j] = the table-wide value id at the rank of percentiles[j] (0..100, else PA_EINVAL; at most
 * PA_MAX_PERCENTILES) in group g, or -1 for a group whose bins are all zero. Replaces
 * PercentileAggregationFunction.extractFinalResult (sort, then values[(int) ((long) size * percentile / 100)], or
 * values[size - 1] at 100): rank = total - 1 when p == 100, else (int64_t)((double)total * p / 100); the result is the
 * first bin whose inclusive prefix sum exceeds the rank (a rank select over the ascending bins, pa_hist.hip).
 * Synchronises `stream`. */
#define PA_MAX_PERCENTILES 64
int pa_query_percentiles(pa_query* q, void* stream, int32_t agg, int64_t num_groups, int32_t num_percentiles,
                         const double* percentiles, int32_t* out_value_ids);

/* The winning rows of LAST / FIRST_ROW_BY_TIME aggregation `agg` for the groups pa_query_fetch returns for the current
 * accumulators, in the same order (num_groups = that call's result): group g's row is doc out_docs[g] of the segment
 * bound at out_segments[g] (int32[num_groups] each, may be NULL); both are -1 for a group with no row (the
 * aggregation-only key 0 when no doc matched). out_cells[c] (int64[num_groups], c < num_columns <=
 * PA_MAX_SELECT_COLUMNS) takes column columns[c] at that row in pa_query_fetch_selection's cell convention: the
 * segment's dictId for a dictionary column, the value of a raw INT / LONG column, the bits of the value as a double for a
 * raw FLOAT / DOUBLE column (0 for a group with no row). The time itself is fetched by listing the time column. Columns
 * must be single-value and not BYTES in every bound segment (PA_EUNSUPPORTED). Replaces
 * {Last,First}WithTimeAggregationFunction.extractAggregationResult / extractGroupByResult (the ValueTimePair the scan's
 * setValueTimePair calls kept): the word decodes to (segment, doc), and one thread per (group, column) reads the cell
 * there (pa_select.hip). Synchronises `stream`. */
int pa_query_fetch_time_rows(pa_query* q, void* stream, int32_t agg, int64_t num_groups, int32_t num_columns,
                             const int32_t* columns, int32_t* out_segments, int32_t* out_docs, int64_t* const* out_cells);

/* How the scan keeps LAST / FIRST_ROW_BY_TIME aggregation `agg`: 1 = packed (one word per group, one scan launch: time
 * bits + row bits <= 63), 2 = wide (a raw time column whose range does not fit: two words and two launches of the scan;
 * everything else the query computes accumulates in the first only), 0 = not such an aggregation, <0 = not prepared or
 * no such aggregation index. Tuning time_rows_wide forces the wide form for raw time columns (pa_tuning.h). */
int32_t pa_query_time_row_form(const pa_query* q, int32_t agg);

/* The reference's intermediate tuples of PA_AGG_MOMENTS aggregation `agg` for the groups pa_query_fetch returns for the
 * current accumulators, in the same order (num_groups = that call's result), as columns: out_count int64[num_groups],
 * out_values[c] double[num_groups] for c < 3 (each pointer may be NULL).
 *   variance    (VarianceTuple.java)    count, out_values = { sum, m2, unused }
 *   covariance  (CovarianceTuple.java)  count, out_values = { sumX, sumY, sumXY }
 * Integer form: the sums are the correctly rounded doubles of the exact integers, and m2 = (n * sum x^2 - (sum x)^2) / n
 * with the numerator exact in 128 bits, rounded once to double, then divided. Double form: sum = S1 + n * pivot,
 * m2 = max(0, S2 - S1 * S1 / n) evaluated with fma; covariance sums as accumulated. A group without docs (the
 * aggregation-only key 0 when no doc matched) gives zeros. One thread per group, one copy per column. Synchronises
 * `stream`. */
int pa_query_fetch_moments(pa_query* q, void* stream, int32_t agg, int64_t num_groups, int64_t* out_count,
                           double* const* out_values);

/* numDocsScanned captured by the last pa_query_fetch (docs that passed the filter; with a multi-value group-by this
 * differs from the sum of the group counts), <0 on error. */
int64_t pa_query_matched_docs(const pa_query* q);

/* numGroupsLimit: 0 if no segment can reach the limit; 1 if the first-position + sort trimming passes run; 2 if the
 * prefix walk runs (SV group-by over a direct key space: limit_walk_kernel + admission inside the scan); <0 if not
 * prepared. */
int32_t pa_query_limit_trimming(const pa_query* q);
/* Segments whose distinct groups reached numGroupsLimit in the last pa_query_fetch (the reference's
 * numGroupsLimitReached is this > 0: GroupByOperator.java:112 per segment, GroupByCombineOperator.java:154 OR), <0 on
 * error. */
int64_t pa_query_num_groups_limit_reached(const pa_query* q);

/* Per-leaf doc bitmaps of one bound segment, for the execution statistics (numEntriesScannedInFilter): the reference
 * counts the docs its filter operators scan (SVScanDocIdIterator.java:76-142: next / advance / applyAnd; AndDocIdSet /
 * OrDocIdSet iterator construction), which depends on which docs each predicate matches and on the segment's indexes,
 * so the host restates that accounting (pinot_amd/filter_stats.py) over these bitmaps. Writes, for every filter leaf l
 * of the spec (pa_query_spec.leaves order), pa_query_leaf_bitmap_words(q, segment) 32-bit words at device_out +
 * l * words: bit (doc & 31) of word (doc >> 5) = the leaf's predicate (with its per-segment negate) on doc.
 * Asynchronous on `stream`. */
int64_t pa_query_leaf_bitmap_words(const pa_query* q, int32_t segment);
int pa_query_leaf_bitmaps(pa_query* q, int32_t segment, uint32_t* device_out, void* stream);

/* Counts over leaf doc bitmaps (pa_query_leaf_bitmaps' layout: leaf l's `words` words at device_bitmaps + l * words,
 * `words` a multiple of 4 covering num_docs)
 * for the execution statistics' closed forms (pinot_amd/filter_stats.py device path), replacing the doc-by-doc replay of
 * the reference's iterators (SVScanDocIdIterator.java:76-142, AndDocIdIterator.java:39-73, AndDocIdSet.java:72-186).
 * prog_a / prog_b: postfix programs over the leaves (a token >= 0 pushes leaf `token`; PA_BIT_AND / PA_BIT_OR pop two
 * masks and push their AND / OR; PA_BIT_NOT complements the top within num_docs; at most PA_BIT_PROG_MAX tokens, stack
 * depth 16, exactly one mask left). ADDS into device_out[0..3] (int64, caller-zeroed): popcount(A), popcount(B),
 * popcount(A & B), and — when len_b > 0 — the leaps of AND(A, B)'s leap-frogging over two scan iterators (labelled
 * docs A-only / B-only / both, in doc order: an A-only doc after a both-doc or at the segment start, or an A-only /
 * B-only doc after the other, starts a leap), from which numEntriesScannedInFilter = num_docs + popcount(A & B) + leaps.
 * device_scratch: pa_bitmap_counts_scratch_bytes(words) bytes. Returns when the counts are written (synchronises
 * `stream`). */
#define PA_BIT_AND (-1)
#define PA_BIT_OR (-2)
#define PA_BIT_NOT (-3)
#define PA_BIT_PROG_MAX 64
int64_t pa_bitmap_counts_scratch_bytes(int64_t words);
int pa_bitmap_counts(const uint32_t* device_bitmaps, int64_t words, int32_t num_leaves, int64_t num_docs,
                     const int32_t* prog_a, int32_t len_a, const int32_t* prog_b, int32_t len_b, void* device_scratch,
                     int64_t* device_out, void* stream);
/* The same counts for many (segment, program A, program B) requests of a prepared query in one pass: the leaf
 * bitmaps of every requested segment (pa_query_leaf_bitmaps) in one launch, then the count kernels for all requests
 * in one launch each. Request r: segments[r], its programs at programs + r * 2 * PA_BIT_PROG_MAX (A, then B at
 * + PA_BIT_PROG_MAX), lengths[2r], lengths[2r + 1] (B may be empty). Writes out[4r .. 4r + 3] (host memory) and
 * returns when they are written (synchronises `stream`). Device scratch is owned by the query. */
int pa_query_filter_counts(pa_query* q, int32_t num_requests, const int32_t* segments, const int32_t* programs,
                           const int32_t* lengths, int64_t* out, void* stream);
/* Execution statistics fused into the scan (PA_QF_FILTER_STATS). When the filter is an AND of two single-value scan
 * leaves, one evaluated on whole tiles (E, sparse) and one per E doc (Z), the scan also counts per segment the docs
 * that matched and the leaps of AndDocIdIterator(A = Z, B = E) (the counts pa_query_filter_counts gives for programs
 * A = [Z], B = [E]): pa_query_leap_leaf returns E's leaf index (spec order) when the scan counts them, else -1.
 * pa_query_leap_counts writes out[3 s .. 3 s + 2] = (matched docs, leaps, 1 if the segment's counts are unavailable:
 * a neighbour search of the fused count gave up) for every bound segment s of the last scan (synchronises `stream`). */
int32_t pa_query_leap_leaf(const pa_query* q);
int pa_query_leap_counts(pa_query* q, int64_t* out, void* stream);

/* Execution statistics of the DataTable (BaseResultsBlock.java:194 puts them in every results block):
 * numEntriesScannedInFilter / numEntriesScannedPostFilter of the bound segments after the last scan.
 *
 * The host passes the filter operator tree the reference builds for each segment (FilterPlanNode +
 * FilterOperatorUtils.getLeafFilterOperator / getAndFilterOperator / getOrFilterOperator: leaf operator choice from the
 * segment's indexes, constant children removed, AND children in reorderAndFilterChildOperators order), as pa_filter_op
 * nodes in pre-order; ops[tree_root[t] ..] is tree t. segment_tree[s] = the tree of bound segment s, or
 * PA_STATS_NON_SCAN (AggregationPlanNode's non-scan plans: neither count), PA_STATS_HOST (the host accounts for the
 * segment itself). The library derives what the reference's iterators read when the projection drives the tree's
 * iterator to the end (SVScanDocIdIterator / MVScanDocIdIterator next, advance and applyAnd; AndDocIdSet's merge of index
 * children; AndDocIdIterator's leap-frog, OrDocIdIterator, NotDocIdIterator) — constants, popcounts of applyAnd chains
 * and leap-frogs counted on the GPU over the segments' leaf bitmaps (pa_stats.hip) — or, when the scan counted a
 * two-scan AND itself (PA_QF_NO_FILTER_STATS unset), those counts.
 * out[0] = numEntriesScannedInFilter over the segments the library covered, out[1] = numEntriesScannedPostFilter =
 * (docs_scanned - docs of PA_STATS_NON_SCAN segments) x projected_columns (docs_scanned: numDocsScanned of the scan,
 * < 0 = the last scan's own counter), out[2] = segments whose count ran on the GPU. segment_in_filter[s]
 * (optional, host int64[num_segments]) = segment s's numEntriesScannedInFilter, or -1 for a segment the host must
 * account for (PA_STATS_HOST, or a tree shape outside the engine: a NOT child of a leap-frogging AND, an AND or NOT
 * child of an OR child of one). Synchronises `stream`. */
#define PA_FOP_EMPTY 0     /* EmptyFilterOperator */
#define PA_FOP_MATCH_ALL 1 /* MatchAllFilterOperator */
#define PA_FOP_SORTED 2    /* SortedIndexBasedFilterOperator (prog: its doc set) */
#define PA_FOP_BITMAP 3    /* BitmapBasedFilterOperator / RangeIndexBasedFilterOperator (exact) */
#define PA_FOP_SCAN 4      /* ScanBasedFilterOperator; mv_column >= 0: over that multi-value column */
#define PA_FOP_AND 5
#define PA_FOP_OR 6
#define PA_FOP_NOT 7
#define PA_STATS_NON_SCAN (-1)
#define PA_STATS_HOST (-2)
typedef struct {
  int32_t kind;          /* PA_FOP_* */
  int32_t num_children;  /* AND / OR: >= 2, NOT: 1, leaves: 0; the children follow in pre-order */
  int32_t mv_column;     /* PA_FOP_SCAN: column id of a multi-value column (-1: single-value) */
  int32_t prog_len;      /* leaves: the operator's doc set as a postfix program over the query's filter leaves */
  int32_t prog[PA_BIT_PROG_MAX];  /* (pa_bitmap_counts tokens) */
} pa_filter_op;
int pa_query_execution_stats(pa_query* q, int32_t num_ops, const pa_filter_op* ops, int32_t num_trees,
                             const int32_t* tree_root, const int32_t* segment_tree, int32_t projected_columns,
                             int64_t docs_scanned, int64_t* out, int64_t* segment_in_filter, void* stream);

/* Cross-GPU merge of hashed key spaces (parallel.merge_hashed_sections around one all-to-all). A row is one slot of
 * every per-key accumulator section (the numDocsScanned counters excluded) in section order: pa_query_row_bytes(q)
 * bytes; the packed key is one of its 8-byte units. pa_query_pack_rows writes the occupied slots (count > 0) as rows
 * grouped by the rank owning their key (a multiplicative hash of the packed key modulo `world`): counts[r] rows for
 * rank r, ranks in order, at device_rows (or, with device_rows NULL, only the counts). pa_query_merge_rows resets the
 * block and merges num_rows rows (from any rank holding the same key space) into it by packed key: SUM for counts
 * and sums, MIN, MAX, byte max for HLL registers and DISTINCTCOUNT presence (GroupByCombineOperator's merge);
 * *groups = the groups now held, *overflow = rows that found no free slot. Both synchronise `stream`. */
int64_t pa_query_row_bytes(const pa_query* q);
int pa_query_pack_rows(pa_query* q, int32_t world, void* device_rows, int64_t* counts, void* stream);
int pa_query_merge_rows(pa_query* q, const void* device_rows, int64_t num_rows, int64_t* groups, int64_t* overflow,
                        void* stream);

/* Group-key layout. Direct (hashed = 0): key = sum_j id_j * prod_{k<j} cardinality_k. Hashed (hashed = 1, chosen when
 * a group-by column is raw or the product of cardinalities is too large to address): the key packs component j
 * (a table-wide key id, or the raw value's bits: 32 for INT/FLOAT, 64 for LONG/DOUBLE) at bit shifts[j]; components
 * wider than 64 bits together take two key words (pa_query_key_words = 2: component j in word shifts[j] / 64 at bit
 * shifts[j] % 64, e.g. GROUP BY two raw LONG columns — NoDictionaryMultiColumnGroupKeyGenerator's composite keys), and
 * pa_query_fetch then writes two int64 per group into out_keys (out_keys holds 2 x capacity). Keys returned by
 * pa_query_fetch follow this layout. */
int pa_query_key_layout(const pa_query* q, int32_t* hashed, int32_t* shifts);
int32_t pa_query_key_words(const pa_query* q);

/* Kernel statistics of the last execute (for roofline accounting): bytes of forward index staged
 * (always-read columns), number of docs scanned. */
int pa_query_stats(const pa_query* q, uint64_t* staged_bytes, uint64_t* num_docs,
                   uint64_t* num_tiles);

/* The kernel plan chosen by pa_query_prepare: accumulator strategy (0 = LDS-privatised, 1 = global atomics,
 * 2 = partitioned: records partitioned by key range, then aggregated per partition in LDS; aggregation-only queries
 * 4..7 = per-lane register accumulators: 4 any column kinds, 5 COUNT only, 6 raw columns only, 7 dictionary
 * columns only; 8 = dense GROUP BY over a small key box, every column staged), 64-doc
 * steps per wave tile, DMA instructions per tile, tile images per wave, workgroups per CU, grid, LDS bytes. */
/* How the main scan pass reads a column (roofline byte model): 1 = staged (every word of every tile streamed through
 * LDS), 0 = read per surviving doc from HBM, -1 = the query does not read it in the main pass. */
int32_t pa_query_column_staged(const pa_query* q, int32_t column_id);
/* Filter literals evaluated on whole staged tiles (the rest only on the docs those matched). */
int32_t pa_query_num_eager_literals(const pa_query* q);
/* 1 if the lane-major scan kernel was chosen (lane l owns docs [32l, 32l+32) of a tile), 0 step-major, <0 error. */
int32_t pa_query_lane_major(const pa_query* q);
/* 1 if the dense GROUP BY kernel accumulates packed words (COUNT + every SUM term in one 64-bit LDS atomic per matching
 * doc, drained per wave into the workgroup's accumulators), 2 if it does so in the kernel specialised to the query's
 * shape (compiled by hiprtc at prepare), 0 if not, <0 error. */
int32_t pa_query_dense_packed(const pa_query* q);
/* 1 when the partitioned plan runs the count-free V emit (each workgroup writes whole record chunks into its own
 * region; pass C reads every partition through its chunk list: no count pass), 2 when it also runs the count-free H
 * emit (DISTINCTCOUNTHLLMV next to the V stream), 0 otherwise, <0 if not prepared. */
int32_t pa_query_count_free_emit(const pa_query* q);
/* 1 when some segment's plan carries the equality prefilter of the lane-major scan (a single `column = value` literal
 * on a staged column of up to 24 bits): in the scan's hoisted steady-state loop whole tiles are first asked "any match?"
 * on the packed stream words. Tiles outside that loop (a wave's first tiles, a segment's ragged last tile, tiles at a
 * segment crossing) take the per-doc leaf as before. 0 otherwise, <0 if not prepared. */
int32_t pa_query_eq_prefilter(const pa_query* q);
/* 1 when the plan sets the nt cache policy for the staged column streams of the lane-major scan's hoisted steady-state
 * loops (by default only a launch that stages more than L2 + Infinity Cache hold). Tiles issued outside those loops (a
 * wave's first tiles, segment crossings, a PA_QF_DEBUG_STREAM_ONLY run) keep the default policy. 0 otherwise, <0 if
 * not prepared. */
int32_t pa_query_stream_nt(const pa_query* q);
/* 1 when the scan runs the kernel compiled for this query's shape by hiprtc at prepare (eqs_jit.hip): one equality on a
 * single-value dictionary column of up to 24 bits as the first clause, every other clause one dictId range read per
 * surviving doc, COUNT / integer SUM over dictionary columns on global accumulators. By default only behind a
 * dictionary of at least 4096 values; tuning eq_jit 0 / 1 turns it off / on wherever the shape fits. The plan's
 * strategy stays that of the generic kernel it restates. 0 otherwise, <0 if not prepared. */
int32_t pa_query_eq_jit(const pa_query* q);
/* Keys per partition of the partitioned plan's V stream (a power of two, or under the count-free emit any count that
 * spreads the key space over whole rounds of pass C's workgroups), 0 when the plan is not partitioned, <0 if not
 * prepared. */
int32_t pa_query_partition_keys(const pa_query* q);
int pa_query_plan(const pa_query* q, int32_t* strategy, int32_t* steps, int32_t* dma_slots, int32_t* ring,
                  int32_t* wg_per_cu, int32_t* grid, int32_t* lds_bytes);

void pa_query_destroy(pa_query* q);

#ifdef __cplusplus
}
#endif

#endif /* PINOT_AMD_H_ */
