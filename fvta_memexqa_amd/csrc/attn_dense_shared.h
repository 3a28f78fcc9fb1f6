// What the dense logit-gradient kernels share (attn_dense.hip: K = 1 rows resident in LDS; attn_cube_bwd.hip: any K, tiled
// over T): the per-channel vectors of the bilinear form read straight from the reference's W layout, and the fold of the
// per-n parameter partials back into that layout.
#pragma once
#include "attn_common.h"

namespace fvta {

__device__ __forceinline__ void dense_vecs(const float* __restrict__ W, int w, int simi, int feat_order, int c, float& U,
                                           float& Rh, float& R2, float& Cq, float& C2) {
  U = Rh = R2 = Cq = C2 = 0.f;
  if (simi == 1) {
    Rh = W[c]; Cq = W[w + c]; U = W[2 * w + c];
  } else if (simi == 2) {
    const float W1 = feat_order == 0 ? W[c] : W[w + c];
    const float W2 = feat_order == 0 ? W[w + c] : W[c];
    U = W1 - 2.f * W2; R2 = W2; C2 = W2;
  } else {
    Rh = W[c]; Cq = W[w + c];
    const float W2 = W[2 * w + c];
    U = W[3 * w + c] - 2.f * W2; R2 = W2; C2 = W2;
  }
}

// fold the per-n partials in n order into dW (the reference's W layout) and db.  grid ceil(w/256) + 1
static __global__ __launch_bounds__(256) void attn_logits_bwd_params_kernel(const float* __restrict__ pvec, const float* __restrict__ pb,
                                                                    float* __restrict__ dW, float* __restrict__ db, int N,
                                                                    int w, int simi, int feat_order) {
  if (blockIdx.x == gridDim.x - 1) {
    if (threadIdx.x == 0) {
      float acc = 0.f;
      for (int n = 0; n < N; ++n) acc += pb[n];
      db[0] += acc;
    }
    return;
  }
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= w) return;
  float v[VEC_COUNT] = {0, 0, 0, 0, 0};
  for (int n = 0; n < N; ++n)
#pragma unroll
    for (int k = 0; k < VEC_COUNT; ++k) v[k] += pvec[((size_t)n * VEC_COUNT + k) * w + c];
  const float dU = v[VEC_U], dRh = v[VEC_RH], dR2 = v[VEC_R2], dCq = v[VEC_CQ], dC2 = v[VEC_C2];
  if (simi == 1) {
    dW[c] += dRh;
    dW[w + c] += dCq;
    dW[2 * w + c] += dU;
  } else if (simi == 2) {
    const float d1 = dU, d2 = -2.f * dU + dR2 + dC2;
    dW[c] += feat_order == 0 ? d1 : d2;
    dW[w + c] += feat_order == 0 ? d2 : d1;
  } else {
    dW[c] += dRh;
    dW[w + c] += dCq;
    dW[2 * w + c] += -2.f * dU + dR2 + dC2;
    dW[3 * w + c] += dU;
  }
}

}  // namespace fvta
