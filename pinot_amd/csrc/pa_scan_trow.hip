// Scan-kernel variants of the row-by-time strategies (FIRSTWITHTIME / LASTWITHTIME: pa_strat_trow.h "row by time"):
// workgroup-private LDS accumulators and device-scope atomics, step-major tiles of 2048 or 1024 docs.
#include "pa_strat_trow.h"

namespace pa {

const void* scan_fn_trow(int strategy, int steps) {
  if (strategy == STRAT_TROW_LDS)
    return steps == 16 ? (const void*)scan_kernel<STRAT_TROW_LDS, 16, 0> : (const void*)scan_kernel<STRAT_TROW_LDS, 32, 0>;
  if (strategy == STRAT_TROW)
    return steps == 16 ? (const void*)scan_kernel<STRAT_TROW, 16, 0> : (const void*)scan_kernel<STRAT_TROW, 32, 0>;
  return nullptr;
}

}  // namespace pa
