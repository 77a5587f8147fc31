// Scan-kernel variants of the filtered-aggregation strategies (AGG(x) FILTER (WHERE ...): pa_strat_filtered.h
// "filtered aggregations"): workgroup-private LDS accumulators and device-scope atomics, step-major tiles of 2048 or 1024
// docs.
#include "pa_strat_filtered.h"

namespace pa {

const void* scan_fn_filtered(int strategy, int steps) {
  if (strategy == STRAT_FILTERED_LDS)
    return steps == 16 ? (const void*)scan_kernel<STRAT_FILTERED_LDS, 16, 0> : (const void*)scan_kernel<STRAT_FILTERED_LDS, 32, 0>;
  if (strategy == STRAT_FILTERED)
    return steps == 16 ? (const void*)scan_kernel<STRAT_FILTERED, 16, 0> : (const void*)scan_kernel<STRAT_FILTERED, 32, 0>;
  return nullptr;
}

}  // namespace pa
