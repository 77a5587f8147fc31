// Scan-kernel variants of aggregation-only queries, lane-major tiles: STRAT_LANE and the COUNT-only
// STRAT_LANE_CNT. The other single-kind variants, lane-major only like _CNT, compile for minutes each and have units of
// their own (pa_scan_lane_raw.hip, pa_scan_lane_dict.hip).
#include "pa_strat_lane.h"

namespace pa {

const void* scan_fn_lane_lm(int strategy, int steps, int lm) {
  if (!lm) return nullptr;
  switch (strategy) {
    case STRAT_LANE: return (const void*)scan_kernel<STRAT_LANE, 32, 1>;
    case STRAT_LANE_CNT: return (const void*)scan_kernel<STRAT_LANE_CNT, 32, 1>;
    default: return nullptr;
  }
}

}  // namespace pa
