// Scan strategy: transform expressions (STRAT_EXPR_LDS / STRAT_EXPR).
// Included by pa_scan_expr.hip in place of pa_scan.h, which declares the entry points it calls and includes no strategy.
#pragma once
#include "pa_scan.h"

namespace pa {

// ---------------------------------------------------------------- expressions (STRAT_EXPR_LDS / STRAT_EXPR)
// SUM(ADD(a, b)), GROUP BY timeConvert(ts, 'MILLISECONDS', 'DAYS'), ...: the reference puts a TransformOperator between
// projection and executor (AggregationPlanNode / GroupByPlanNode), and the aggregation functions and
// NoDictionary{Single,Multi}ColumnGroupKeyGenerator read its block values. Here a matching doc of a 64-doc step takes
// two phases:
//   gather    every distinct operand column of the query's expressions (ExprDesc::col_slot) is read once: first every
//             dictionary column's dictId (staged image or HBM) and every raw column's value, then every dictionary
//             gather — independent loads, issued back to back, so the step pays one HBM latency per phase, not one per
//             operand. A value is kept as 64 bits in its family: int64 (INT / LONG) or double (FLOAT widened / DOUBLE).
//   evaluate  the programs (ExprProg) run over eight 64-bit value registers. The program is wave-uniform and read with
//             scalar loads, so the opcode dispatch is scalar control flow; the lanes differ only in their values.
// Registers, column values and results are small arrays touched only with compile-time indices (a select chain per
// access with the uniform runtime index: expr_get / expr_set), so they stay in VGPRs: no scratch memory, whose
// accesses would wait behind the DMA ring.
// A DOUBLE result aggregates as SRC_DOUBLE, a LONG result as SRC_LONG (agg_apply_set, the equal-key sets of
// accumulate_step); a group-by expression contributes its 64 result bits (NaNs made one: doubleToLongBits) as a raw
// LONG / DOUBLE column does, so such a query's key space is hashed.

// Java's (long) cast of a double: NaN -> 0, saturating.
__device__ __forceinline__ int64_t java_d2l(double d) {
  if (d != d) return 0;
  if (d >= 9223372036854775808.0) return INT64_MAX;
  if (d <= -9223372036854775808.0) return INT64_MIN;
  return (int64_t)d;
}

// TimeUnit.convert to a finer unit: d * m saturating at Long.MIN_VALUE / MAX_VALUE (m > 0).
__device__ __forceinline__ int64_t tconv_mul(int64_t d, int64_t m) {
  const int64_t over = INT64_MAX / m;
  if (d > over) return INT64_MAX;
  if (d < -over) return INT64_MIN;
  return d * m;
}

// (expr_get / expr_set, the mask chains over the eight-element arrays: in pa_scan.h above accumulate_step, which reads
// the results)
static_assert(PA_MAX_EXPR_REGS == PA_MAX_EXPR_COLUMNS && PA_MAX_EXPR_REGS == PA_MAX_EXPRS,
              "expr_get / expr_set serve the registers, the column values and the results");

// Gather phase: cv[c] = the doc's value of operand column c (int64, or a double's bits); bit c of the returned mask:
// the column is FLOAT / DOUBLE in this segment (wave-uniform). Lanes outside `in` load nothing and hold zeros.
__device__ __forceinline__ uint32_t expr_gather(const ExprDesc* __restrict__ E, const DevSeg* __restrict__ seg,
                                                const uint32_t* img, int doc_local, int64_t doc, bool in,
                                                uint64_t (&cv)[PA_MAX_EXPR_COLUMNS]) {
  const int nc = E->num_cols;
  uint32_t fmask = 0;
  uint32_t id[PA_MAX_EXPR_COLUMNS];
#pragma unroll
  for (int c = 0; c < PA_MAX_EXPR_COLUMNS; ++c) {
    cv[c] = 0;
    id[c] = 0;
    if (c >= nc) continue;
    const DevCol& col = seg->cols[E->col_slot[c]];
    if (col.vtype == PA_FLOAT || col.vtype == PA_DOUBLE) fmask |= 1u << c;
    if (!in) continue;
    if (col.kind == COL_SV_DICT) {
      id[c] = decode_dict_id(col, img, doc_local, doc);
    } else {
      switch (col.vtype) {
        case PA_INT: cv[c] = (uint64_t)(int64_t)gp((const int32_t*)col.raw)[doc]; break;
        case PA_LONG: cv[c] = (uint64_t)gp((const int64_t*)col.raw)[doc]; break;
        case PA_FLOAT: cv[c] = __builtin_bit_cast(uint64_t, (double)gp((const float*)col.raw)[doc]); break;
        default: cv[c] = (uint64_t)gp((const int64_t*)col.raw)[doc]; break;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < PA_MAX_EXPR_COLUMNS; ++c) {
    if (c >= nc || !in) continue;
    const DevCol& col = seg->cols[E->col_slot[c]];
    if (col.kind != COL_SV_DICT) continue;
    // (dict_i64 holds int64 values, dict_f64 doubles: 64 bits of the column's family either way)
    cv[c] = ((fmask >> c) & 1u) ? (uint64_t)gp((const int64_t*)col.dict_f64)[id[c]] : (uint64_t)gp(col.dict_i64)[id[c]];
  }
  return fmask;
}

// Evaluate phase: one program over the gathered values; returns the result's 64 bits (a double's, or the int64).
__device__ __forceinline__ uint64_t expr_eval(const ExprProg& P, const uint64_t (&cv)[PA_MAX_EXPR_COLUMNS],
                                              uint32_t fmask) {
  uint64_t r[PA_MAX_EXPR_REGS];
#pragma unroll
  for (int k = 0; k < PA_MAX_EXPR_REGS; ++k) r[k] = 0;
  uint64_t last = 0;
  const int n = P.num_ops;
  for (int o = 0; o < n; ++o) {
    const ExprOp& X = P.ops[o];
    const int op = X.op;
    uint64_t out;
    if (op == PA_EXPR_LOAD_COL) {
      const uint64_t x = expr_get(cv, X.a);
      const bool fl = (fmask >> X.a) & 1u;
      if (X.b == PA_EXPR_DOUBLE)
        out = fl ? x : __builtin_bit_cast(uint64_t, (double)(int64_t)x);
      else
        out = fl ? (uint64_t)java_d2l(__builtin_bit_cast(double, x)) : x;
    } else {
      const uint64_t ab = X.a_kind == PA_EXPR_ARG_REG ? expr_get(r, X.a) : (uint64_t)X.a_imm;
      if (op <= PA_EXPR_MOD) {
        const uint64_t bb = X.b_kind == PA_EXPR_ARG_REG ? expr_get(r, X.b) : (uint64_t)X.b_imm;
        const double a = __builtin_bit_cast(double, ab), b = __builtin_bit_cast(double, bb);
        double d;
        if (op == PA_EXPR_ADD) d = a + b;
        else if (op == PA_EXPR_SUB) d = a - b;
        else if (op == PA_EXPR_MUL) d = a * b;
        else if (op == PA_EXPR_DIV) d = a / b;
        else d = fmod(a, b);
        out = __builtin_bit_cast(uint64_t, d);
      } else if (op == PA_EXPR_ABS) {
        out = ab & 0x7fffffffffffffffull;
      } else if (op == PA_EXPR_CEIL) {
        out = __builtin_bit_cast(uint64_t, ceil(__builtin_bit_cast(double, ab)));
      } else if (op == PA_EXPR_FLOOR) {
        out = __builtin_bit_cast(uint64_t, floor(__builtin_bit_cast(double, ab)));
      } else if (op == PA_EXPR_D2L) {
        out = (uint64_t)java_d2l(__builtin_bit_cast(double, ab));
      } else if (op == PA_EXPR_L2D) {
        out = __builtin_bit_cast(uint64_t, (double)(int64_t)ab);
      } else if (op == PA_EXPR_TCONV_DIV) {
        out = (uint64_t)((int64_t)ab / X.b_imm);
      } else {
        out = (uint64_t)tconv_mul((int64_t)ab, X.b_imm);
      }
    }
    expr_set(r, X.dst, out);
    last = out;
  }
  return last;
}

// One 64-doc step of a query with expressions: gather, evaluate every program, then accumulate_step with the results.
template <int STRAT>
__device__ __forceinline__ void expr_step(const DevQuery* __restrict__ q, const DevSeg* __restrict__ seg,
                                          const uint32_t* img, int doc_local, int64_t doc, uint64_t matched, int lane,
                                          const Acc<STRAT>& acc) {
  ExprVals ev;
  ev.E = uniform_ptr(q->expr);
  const bool mine = (matched >> lane) & 1ull;
  uint64_t cv[PA_MAX_EXPR_COLUMNS];
  const uint32_t fmask = expr_gather(ev.E, seg, img, doc_local, doc, mine, cv);
  const int ne = ev.E->num_exprs;
#pragma unroll
  for (int e = 0; e < PA_MAX_EXPRS; ++e) ev.res[e] = 0;
  for (int e = 0; e < ne; ++e) {  // (not unrolled: one copy of the evaluator in the kernel)
    uint64_t x = expr_eval(ev.E->progs[e], cv, fmask);
    // (one NaN: doubleToLongBits, for the group key; SUM / MIN / MAX treat every NaN alike)
    if (ev.E->progs[e].result_type == PA_EXPR_DOUBLE && (x & 0x7fffffffffffffffull) > 0x7ff0000000000000ull)
      x = 0x7ff8000000000000ull;
    expr_set(ev.res, e, x);
  }
  accumulate_step<STRAT>(q, seg, img, doc_local, doc, matched, lane, acc, &ev);
}

}  // namespace pa
