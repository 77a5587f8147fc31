// Scan-kernel variants of the standard GROUP BY strategy, STRAT_LDS: workgroup-private accumulators in LDS, flushed at
// the end of the kernel (global atomics: pa_scan_global.hip; per-lane accumulators: pa_scan_lane_*.hip).
#include "pa_scan.h"

namespace pa {

const void* scan_fn_std(int strategy, int steps, int lm) {
  if (strategy != STRAT_LDS) return nullptr;
  if (lm) return (const void*)scan_kernel<STRAT_LDS, 32, 1>;
  return steps == 16 ? (const void*)scan_kernel<STRAT_LDS, 16, 0> : (const void*)scan_kernel<STRAT_LDS, 32, 0>;
}

}  // namespace pa
