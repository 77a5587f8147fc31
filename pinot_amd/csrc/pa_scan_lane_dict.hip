// Scan-kernel variant of aggregation-only queries over dictionary columns only (STRAT_LANE_DICT):
// lane-major.
#include "pa_strat_lane.h"

namespace pa {

const void* scan_fn_lane_dict(int strategy, int steps, int lm) {
  return strategy == STRAT_LANE_DICT && lm ? (const void*)scan_kernel<STRAT_LANE_DICT, 32, 1> : nullptr;
}

}  // namespace pa
