// From the gradients of the bilinear form's five per-channel vectors (attn_common.h: U, Rh, R2, Cq, C2) to the gradient of
// att_logits/W in its own feature order -- the inverse of attn_vecs_kernel.  One copy for attn_bwd.hip and
// attn_shared_bwd.hip.  dW is accumulated into.
#pragma once
#include "attn_common.h"

namespace fvta {

#ifdef __HIPCC__
__device__ __forceinline__ void attn_bwd_add_dW(int simi, int feat_order, int w, int c, float dU, float dRh, float dR2,
                                                float dCq, float dC2, float* __restrict__ dW) {
  if (simi == 1) {
    dW[c] += dRh;
    dW[w + c] += dCq;
    dW[2 * w + c] += dU;
  } else if (simi == 2) {
    const float d1 = dU, d2 = -2.f * dU + dR2 + dC2;
    dW[c] += feat_order == 0 ? d1 : d2;
    dW[w + c] += feat_order == 0 ? d2 : d1;
  } else if (simi == 3) {
    dW[c] += dRh;
    dW[w + c] += dCq;
    dW[2 * w + c] += -2.f * dU + dR2 + dC2;
    dW[3 * w + c] += dU;
  }
}
#endif

}  // namespace fvta
