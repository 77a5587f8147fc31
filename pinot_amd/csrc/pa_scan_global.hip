// Scan-kernel variants of STRAT_GLOBAL: device-scope atomics on the global accumulators (Acc in pa_scan.h).
#include "pa_scan.h"

namespace pa {

const void* scan_fn_global(int strategy, int steps, int lm) {
  if (strategy != STRAT_GLOBAL) return nullptr;
  if (lm) return (const void*)scan_kernel<STRAT_GLOBAL, 32, 1>;
  return steps == 16 ? (const void*)scan_kernel<STRAT_GLOBAL, 16, 0> : (const void*)scan_kernel<STRAT_GLOBAL, 32, 0>;
}

}  // namespace pa
