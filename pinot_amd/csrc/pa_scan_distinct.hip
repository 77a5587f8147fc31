// Scan-kernel variants of the distinct strategies (SELECT DISTINCT ...: pa_strat_distinct.h "distinct"): the LDS bitmap and the
// global bitmap, step-major tiles of 2048 or 1024 docs.
#include "pa_strat_distinct.h"

namespace pa {

const void* scan_fn_distinct(int strategy, int steps) {
  if (strategy == STRAT_DISTINCT_LDS)
    return steps == 16 ? (const void*)scan_kernel<STRAT_DISTINCT_LDS, 16, 0> : (const void*)scan_kernel<STRAT_DISTINCT_LDS, 32, 0>;
  if (strategy == STRAT_DISTINCT)
    return steps == 16 ? (const void*)scan_kernel<STRAT_DISTINCT, 16, 0> : (const void*)scan_kernel<STRAT_DISTINCT, 32, 0>;
  return nullptr;
}

}  // namespace pa
