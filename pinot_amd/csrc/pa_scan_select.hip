// Scan-kernel variants of the selection strategy (SELECT ... ORDER BY ... LIMIT: pa_strat_select.h "selection"): step-major
// tiles of 2048 or 1024 docs.
#include "pa_strat_select.h"

namespace pa {

const void* scan_fn_select(int strategy, int steps) {
  if (strategy != STRAT_SELECT) return nullptr;
  return steps == 16 ? (const void*)scan_kernel<STRAT_SELECT, 16, 0> : (const void*)scan_kernel<STRAT_SELECT, 32, 0>;
}

}  // namespace pa
