// Scan-kernel variants of aggregation-only queries, step-major tiles of 2048 or 1024 docs: STRAT_LANE.
#include "pa_strat_lane.h"

namespace pa {

const void* scan_fn_lane_sm(int strategy, int steps, int lm) {
  if (strategy != STRAT_LANE || lm) return nullptr;  // (the single-kind variants are lane-major only)
  return steps == 16 ? (const void*)scan_kernel<STRAT_LANE, 16, 0> : (const void*)scan_kernel<STRAT_LANE, 32, 0>;
}

}  // namespace pa
