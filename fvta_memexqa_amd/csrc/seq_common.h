// What the row-owned recurrences share (attgru_seq.hip, gru_seq.hip): a workgroup owns SEQ_RT = 16 rows of the batch for a
// whole call (the M of v_mfma_f32_16x16x4_f32, exact fp32), so row n's chain never waits for another workgroup.  Here are
// the tile constants, the lane bookkeeping of the MFMA C layout, the LDS staging of the per-step regime, the MFMA loops
// over LDS images, and the host side the launchers have in common: the regime test, the grids, the carvers of `saved` and
// the workspace, the plan words and the fill of the parameter gradients.  A cell keeps its gate math, how it holds its
// weights in the one-launch regime, and its entry points.  Every device helper is inlined; check a kernel's registers and
// its speed when it starts to use one (gru_seq.hip's one-launch kernels keep their preamble written out for that reason).
// Rounding: a cell spells the fused multiply-adds of its state update out (fmaf).  Left to the compiler, the TRAIN and the
// inference instantiation of a kernel contract a * b + c differently, and the two then differ in the last bit.
#pragma once
#include "fvta_common.h"

namespace fvta {

constexpr int SEQ_RT = 16;          // rows of a workgroup tile
constexpr int SEQ_A_WAVES = 8;      // one-launch regime: at most one wave per 16 units, 512 threads
constexpr int SEQ_A_DP_MAX = 16 * SEQ_A_WAVES;
constexpr int SEQ_B_KC = 32;        // per-step regime: k-chunk staged through LDS
constexpr int SEQ_B_CT = 64;        // per-step regime: units per workgroup (4 waves x 16)
constexpr int SEQ_B_LD = SEQ_B_KC + 2;

// ---- lane bookkeeping: in the MFMA C layout a lane holds rows i0 .. i0 + 3 of unit u (c0: the workgroup's first unit)
struct SeqLane { int u, i0; };
__device__ __forceinline__ SeqLane seq_lane(int wave, int lane, int c0 = 0) { return {c0 + wave * 16 + (lane & 15), 4 * (lane >> 4)}; }
// is element (n, u) on the [N, d] tensor: the guard of a per-step epilogue
__device__ __forceinline__ bool seq_live(int n, int u, int N, int d) { return n < N && u < d; }
// the lane's four rows of the tile at m0: ok where (row, u) is on the tensor, row clamped to 0 past N (a safe address)
__device__ __forceinline__ void seq_lane_rows(int m0, int i0, int u, int N, int d, bool (&ok)[4], int64_t (&row)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = m0 + i0 + r;
    ok[r] = seq_live(n, u, N, d);
    row[r] = n < N ? n : 0;
  }
}
// the lane's four values to rows of dst [N, d] (NULL: nothing): h_last, d_h0
__device__ __forceinline__ void seq_store_rows(float* dst, const float (&v)[4], const bool (&ok)[4], const int64_t (&row)[4], int d,
                                               int u) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (dst && ok[r]) dst[row[r] * d + u] = v[r];
}

// ---- staging of the per-step regime (256 threads, images of row stride SEQ_B_LD)
// element (i, kk) of a [.][32] image that thread tid writes in pass p: 8 rows a pass
__device__ __forceinline__ void seq_b_decode(int tid, int p, int& i, int& kk) { i = (tid + p * 256) >> 5; kk = tid & 31; }
// the A tile [16][32] <- columns k0.. of rows m0.. of a dense [N, ld] matrix (NULL: zeros); zero off the tensor
__device__ __forceinline__ void seq_stage_a(float* A_l, const float* __restrict__ src, int64_t ld, int N, int d, int m0, int k0,
                                            int tid) {
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    int i, kk;
    seq_b_decode(tid, p, i, kk);
    const int n = m0 + i, k = k0 + kk;
    float v = 0.f;
    if (src && n < N && k < d) v = src[(int64_t)n * ld + k];
    A_l[i * SEQ_B_LD + kk] = v;
  }
}
// Weight images [64][32] of a [d][d] block W of row stride ldw: image[c][kk] = W[k0 + kk][c0 + c] (ALONG_K = false: the
// forward product, consecutive threads read along c) or W[c0 + c][k0 + kk] (true: the transposed product, along k).
// Returns the source offset of the element thread tid writes in pass p -- 0, a safe address, where it is off W -- and its
// place in the image.
template <bool ALONG_K>
__device__ __forceinline__ size_t seq_w_src(int tid, int p, size_t ldw, int d, int c0, int k0, int& dst, bool& ok) {
  const int idx = tid + p * 256;
  const int c = ALONG_K ? idx >> 5 : idx & 63, kk = ALONG_K ? idx & 31 : idx >> 6;
  const int u = c0 + c, k = k0 + kk;
  ok = u < d && k < d;
  dst = c * SEQ_B_LD + kk;
  return ok ? (ALONG_K ? (size_t)u * ldw + k : (size_t)k * ldw + u) : 0;
}
template <bool ALONG_K>
__device__ __forceinline__ void seq_stage_w1(float* B_l, const float* __restrict__ W, size_t ldw, int d, int c0, int k0, int tid) {
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    int dst;
    bool ok;
    const size_t src = seq_w_src<ALONG_K>(tid, p, ldw, d, c0, k0, dst, ok);
    B_l[dst] = ok ? W[src] : 0.f;
  }
}
template <bool ALONG_K>   // two blocks of one row stride
__device__ __forceinline__ void seq_stage_w2(float* B0_l, float* B1_l, const float* __restrict__ W0, const float* __restrict__ W1,
                                             size_t ldw, int d, int c0, int k0, int tid) {
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    int dst;
    bool ok;
    const size_t src = seq_w_src<ALONG_K>(tid, p, ldw, d, c0, k0, dst, ok);
    const float v0 = W0[src], v1 = W1[src];
    B0_l[dst] = ok ? v0 : 0.f;
    B1_l[dst] = ok ? v1 : 0.f;
  }
}

// ---- acc += A[16][K] * B[16][K]^T for LDS images whose rows are k-contiguous (ld = 2 mod 32: lanes 0..31 hit 32 banks).
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

// ---- host side
// a size query's answer to a bad descriptor: 0, with the message set
static inline size_t seq_refuse(const char* msg) { return fvta_set_error("%s", msg), 0; }
static inline int seq_dp(int d) { return (d + 15) / 16 * 16; }
static inline bool seq_regime_a(int d) { return seq_dp(d) <= SEQ_A_DP_MAX; }
static inline unsigned seq_row_tiles(int N) { return (unsigned)((N + SEQ_RT - 1) / SEQ_RT); }
static inline dim3 seq_grid_b(int N, int d) { return dim3(seq_row_tiles(N), (unsigned)((d + SEQ_B_CT - 1) / SEQ_B_CT)); }

struct SeqSaved {  // what a training forward keeps: four arrays of n = rows * steps * d floats
  float* s[4];
  size_t bytes;
  SeqSaved(size_t n, void* p) {
    FvtaCarver c(p);
    for (float*& q : s) q = c.take<float>(n);
    bytes = c.off;
  }
};
struct SeqWork {  // a of ka * n floats, b of n, c of n (only if `third`), then two state rows of nd = rows * d
  float *a, *b, *c, *s0, *s1;
  size_t bytes;
  SeqWork(size_t n, size_t nd, int ka, bool third, void* p) {
    FvtaCarver cv(p);
    a = cv.take<float>(ka * n);
    b = cv.take<float>(n);
    c = third ? cv.take<float>(n) : nullptr;
    s0 = cv.take<float>(nd);
    s1 = cv.take<float>(nd);
    bytes = cv.off;
  }
};

// the four words of a plan: regime (0 = A: the recurrence is one launch; 1 = B: per_step launches for each of `steps`), the
// launches of a forward (the two hoisted products, then the recurrence) and of a backward (the fill of an accumulate = 0
// call, the recurrence, fvta_linear_bwd's six kernels), the rows of a workgroup tile
static inline void seq_fill_plan(int32_t* out, bool A, int per_step, int steps) {
  const int rec = A ? 1 : per_step * steps;
  out[0] = A ? 0 : 1;
  out[1] = 2 + rec;
  out[2] = 1 + rec + 6;
  out[3] = SEQ_RT;
}

// The parameter gradients of an `accumulate = 0` backward start at zero (fvta_linear_bwd adds): one launch zeroes up to
// five buffers (unused entries: n = 0).  The kernel lives in attgru_seq.hip.
struct SeqZeroTable {
  float* p[5];
  int64_t n[5];
};
void seq_zero_params(const SeqZeroTable& t, hipStream_t s);

}  // namespace fvta
