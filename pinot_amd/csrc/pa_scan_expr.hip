// Scan-kernel variants of the transform-expression strategies (SUM(ADD(a, b)), GROUP BY timeConvert(...):
// pa_strat_expr.h "expressions"): workgroup-private LDS accumulators and device-scope atomics, step-major tiles of 2048
// or 1024 docs.
#include "pa_strat_expr.h"

namespace pa {

const void* scan_fn_expr(int strategy, int steps) {
  if (strategy == STRAT_EXPR_LDS)
    return steps == 16 ? (const void*)scan_kernel<STRAT_EXPR_LDS, 16, 0> : (const void*)scan_kernel<STRAT_EXPR_LDS, 32, 0>;
  if (strategy == STRAT_EXPR)
    return steps == 16 ? (const void*)scan_kernel<STRAT_EXPR, 16, 0> : (const void*)scan_kernel<STRAT_EXPR, 32, 0>;
  return nullptr;
}

}  // namespace pa
