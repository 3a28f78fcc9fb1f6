// What the row-owned recurrences share (attgru_seq.hip, gru_seq.hip): a workgroup owns SEQ_RT = 16 rows of the batch for a
// whole call (the M of v_mfma_f32_16x16x4_f32, exact fp32), so row n's chain never waits for another workgroup.  Here are
// the tile constants and the MFMA loops over LDS images; the cells and their launchers stay in the two files.
#pragma once
#include "fvta_common.h"

namespace fvta {

constexpr int SEQ_RT = 16;          // rows of a workgroup tile
constexpr int SEQ_B_KC = 32;        // per-step regime: k-chunk staged through LDS
constexpr int SEQ_B_CT = 64;        // per-step regime: units per workgroup (4 waves x 16)
constexpr int SEQ_B_LD = SEQ_B_KC + 2;

// acc += A[16][K] * B[16][K]^T for LDS images whose rows are k-contiguous (ld = 2 mod 32: lanes 0..31 hit 32 banks).
// lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15] = image[j][k]
__device__ __forceinline__ void seq_mma1(const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb, int K,
                                         int lane, f32x4& acc) {
  const float* ap = A + (lane & 15) * lda + (lane >> 4);
  const float* bp = B + (lane & 15) * ldb + (lane >> 4);
  for (int k0 = 0; k0 < K; k0 += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[k0], bp[k0], acc, 0, 0, 0);
}
__device__ __forceinline__ void seq_mma2(const float* __restrict__ A, int lda, const float* __restrict__ B0,
                                         const float* __restrict__ B1, int ldb, int K, int lane, f32x4& acc0, f32x4& acc1) {
  const float* ap = A + (lane & 15) * lda + (lane >> 4);
  const float* b0 = B0 + (lane & 15) * ldb + (lane >> 4);
  const float* b1 = B1 + (lane & 15) * ldb + (lane >> 4);
  for (int k0 = 0; k0 < K; k0 += 4) {
    const float av = ap[k0];
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0[k0], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1[k0], acc1, 0, 0, 0);
  }
}
__device__ __forceinline__ void seq_mma_ab(const float* __restrict__ A0, const float* __restrict__ A1, int lda,
                                           const float* __restrict__ B0, const float* __restrict__ B1, int ldb, int K,
                                           int lane, f32x4& acc0, f32x4& acc1) {
  const int o = (lane & 15) * lda + (lane >> 4), ob = (lane & 15) * ldb + (lane >> 4);
  for (int k0 = 0; k0 < K; k0 += 4) {
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(A0[o + k0], B0[ob + k0], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(A1[o + k0], B1[ob + k0], acc1, 0, 0, 0);
  }
}

}  // namespace fvta
