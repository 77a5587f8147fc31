// Scan-kernel variants of the moment strategies (VAR_POP / STDDEV / COVAR: pa_strat_moments.h "moments"):
// workgroup-private LDS accumulators and device-scope atomics, step-major tiles of 2048 or 1024 docs.
#include "pa_strat_moments.h"

namespace pa {

const void* scan_fn_moments(int strategy, int steps) {
  if (strategy == STRAT_MOM_LDS)
    return steps == 16 ? (const void*)scan_kernel<STRAT_MOM_LDS, 16, 0> : (const void*)scan_kernel<STRAT_MOM_LDS, 32, 0>;
  if (strategy == STRAT_MOM)
    return steps == 16 ? (const void*)scan_kernel<STRAT_MOM, 16, 0> : (const void*)scan_kernel<STRAT_MOM, 32, 0>;
  return nullptr;
}

}  // namespace pa
