// Scan-kernel variant of aggregation-only queries over raw columns only (STRAT_LANE_RAW): lane-major.
#include "pa_strat_lane.h"

namespace pa {

const void* scan_fn_lane_raw(int strategy, int steps, int lm) {
  return strategy == STRAT_LANE_RAW && lm ? (const void*)scan_kernel<STRAT_LANE_RAW, 32, 1> : nullptr;
}

}  // namespace pa
