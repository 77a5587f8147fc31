// Dispatch of the scan kernel: the kernel pointer of a (strategy, steps, layout) from the pa_scan_*.hip unit holding
// it, and the launch, LDS limit and occupancy calls on it.
#include <initializer_list>
#include "pa_launch.h"

namespace pa {

static const void* scan_fn(int strategy, int steps, int lm) {
  for (auto get : {scan_fn_std, scan_fn_global, scan_fn_lane_lm, scan_fn_lane_raw, scan_fn_lane_dict, scan_fn_lane_sm})
    if (const void* f = get(strategy, steps, lm)) return f;
  if (const void* f = scan_fn_gdense(strategy, lm)) return f;
  if (const void* f = scan_fn_select(strategy, steps)) return f;
  if (const void* f = scan_fn_distinct(strategy, steps)) return f;
  if (const void* f = scan_fn_filtered(strategy, steps)) return f;
  if (const void* f = scan_fn_expr(strategy, steps)) return f;
  if (const void* f = scan_fn_trow(strategy, steps)) return f;
  if (const void* f = scan_fn_moments(strategy, steps)) return f;
  if (const void* f = scan_fn_part_a(strategy)) return f;
  if (const void* f = scan_fn_part_mv(strategy)) return f;
  return scan_fn_part_b(strategy);
}

hipError_t set_scan_lds_limit(int strategy, int steps, int lm, int bytes) {
  return hipFuncSetAttribute(scan_fn(strategy, steps, lm), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

hipError_t scan_occupancy(int strategy, int steps, int lm, int lds_bytes, int* blocks_per_cu) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, scan_fn(strategy, steps, lm), scan_waves(strategy) * kWave,
                                                      (size_t)lds_bytes);
}

hipError_t launch_scan(int strategy, int steps, int lm, int grid, int lds_bytes, const DevQuery* q, const DevSeg* segs,
                       const LmSegPlan* plans, const PartScratch& ps, hipStream_t s) {
  PartScratch pcopy = ps;
  void* args[] = {(void*)&q, (void*)&segs, (void*)&plans, (void*)&pcopy};
  return hipLaunchKernel(scan_fn(strategy, steps, lm), dim3(grid), dim3(scan_waves(strategy) * kWave), args,
                         (size_t)lds_bytes, s);
}

}  // namespace pa
