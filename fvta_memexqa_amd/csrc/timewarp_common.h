// What the time warp's kernels (timewarp.hip) and the shared-context attention under the warp (attn_shared.hip) agree on.
#pragma once
#include "fvta_common.h"

namespace fvta {

// cnt(t) = #{t' allowed by warp_type around t}: the row sums of time_indication_func's 0/1 factor (model_v2.py:301-341)
__device__ __forceinline__ float tw_count(int t, int T, int warp_type, int win) {
  switch (warp_type) {
    case 1: return (float)T;            // all time (model_v2.py:303-304)
    case 2: return 1.f;                 // diagonal (312-314)
    case 3: return (float)(t + 1);      // past, lower triangular (315-323)
    case 4: return (float)(T - t);      // future (324-330)
    default: return (float)(min(t + win, T - 1) - max(t - win, 0) + 1);  // 5: band of half-width ceil(window_t) (332-339)
  }
}

}  // namespace fvta
