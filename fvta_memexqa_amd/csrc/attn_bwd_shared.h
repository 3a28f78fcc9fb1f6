// Shared by the focal-attention backward kernels (attn_bwd.hip, attn_shared_bwd.hip, attn_dense.hip, attn_cube_bwd.hip) --
// the counterpart of attn_fwd_shared.h: the per-(item, k) scalars of the prep kernels, the "slots in order, eight loads in
// flight" sum, the fold of the dQs / d ct partials into d_hq and the parameter-vector partials, the pieces of the parameter
// kernels (bias block, strided row sum, four-way combine into dW), the fp64 block sum, and the declaration of the dense
// paths' parameter kernel.  The W mapping itself (attn_vecs_of, attn_bwd_add_dW) is in attn_common.h: the forward uses it too.
// Every helper is inlined; every sum keeps one fixed order (no atomics: two runs are bitwise equal).
#pragma once
#include "attn_common.h"

namespace fvta {

constexpr int ATTN_BWD_JG = 8;  // question positions per workgroup of a fold: two per wave (four, one per wave: no faster)

// ---- per-(item, k) scalars of one item (an n of attn_bwd.hip, a question of attn_shared_bwd.hip); the pointers are the
// item's own: g [w], u [K,w], M / r / L [K], amax [K,T] -> coef = r / L, gu = g.u[k], dss = ds[k] / (#t with amax == M).
// A wave per k (no workgroup barrier inside the k loop; 16 waves: a stream's dot product and tie count are one chain of
// load latencies, 10 streams per wave took 20 us at K = 40); then thread k finishes stream k (one thread walking all K with
// three dependent global loads each: ~20 of the launch's 25 us), the mean summed in k order by every thread from LDS.
// `allmasked`: stream threadIdx.x passes nothing into its masked logits.  Each forward states that fact its own way
// (fvta_attn_fwd: sv.allmasked, no valid (t, j) pair; the shared forward keeps no such flag, there M == -1e30 says it):
// the predicate stays with the caller.
__device__ __forceinline__ void attn_bwd_prep_body(const float* __restrict__ g, const float* __restrict__ u,
                                                   const float* __restrict__ M, const float* __restrict__ amax,
                                                   const float* __restrict__ r, const float* __restrict__ L, bool allmasked,
                                                   int w, int K, int T, float* __restrict__ coef, float* __restrict__ gu,
                                                   float* __restrict__ dss) {
  __shared__ float s_gu[64], s_r[64];
  __shared__ int s_ties[64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int k = wave; k < K; k += (int)(blockDim.x >> 6)) {
    const float* uk = u + (size_t)k * w;
    float acc = 0.f;
    for (int c = lane; c < w; c += 64) acc += g[c] * uk[c];
    acc = wave_sum(acc);
    const float Mk = M[k];
    const float* am = amax + (size_t)k * T;
    int ties = 0;
    for (int t = lane; t < T; t += 64) ties += (am[t] == Mk) ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ties += __shfl_xor(ties, o, 64);
    if (lane == 0) {
      s_gu[k] = acc;
      s_ties[k] = ties;
    }
  }
  float rk = 0.f, Lk = 1.f;
  if (tid < K) {
    rk = r[tid];
    Lk = L[tid];
    s_r[tid] = rk;
  }
  __syncthreads();
  if (tid < K) {
    float mean = 0.f;
    for (int k = 0; k < K; ++k) mean += s_r[k] * s_gu[k];
    coef[tid] = rk / Lk;
    gu[tid] = s_gu[tid];
    const float ds = rk * (s_gu[tid] - mean);
    dss[tid] = allmasked ? 0.f : ds / (float)max(1, s_ties[tid]);
  }
}

// ---- ld(0) + ld(1) + ... + ld(n - 1), added in that order, eight loads in flight (one dependent load after the other:
// 105 us for the dQs fold at the metric shape, 0.6 TB/s)
template <class V, class LD>
__device__ __forceinline__ V attn_bwd_slot_sum(int n, LD ld) {
  V acc = V{};
  int i = 0;
  for (; i + 8 <= n; i += 8) {
    V v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = ld(i + u);
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += v[u];
  }
  for (; i < n; ++i) acc += ld(i);
  return acc;
}

__device__ __forceinline__ f32x4 ld4_if(bool live, const float* p) { return live ? ld4(p) : zero4(); }

// ---- fold of one item's dQs / d ct partials.  grid (items, ceil(w / 256), ceil(JQ / 8)), 256 threads: a block takes 8
// question positions x 256 channels; a lane owns the 4 channels from c = blockIdx.y * 256 + 4 * lane (16-byte loads; w is a
// multiple of 4: they are inside or outside together), wave v the positions j_lo + v and j_lo + v + 4.
//   dct[j] = the item's `nslot` d ct slots dctp[i * dct_stride + j] in slot order (block (., 0, 0) also leaves it in dctn)
//   d_hq[j] (+)= U dQ_of(j) + dct[j] (Cq + 2 C2 q[j])          hq / d_hq / dctn: the item's own [JQ,w], [JQ,w], [JP]
//   pU = sum_j dQ q, pCq = sum_j dct q, pC2 = sum_j dct q^2    over the block's positions; waves 1..3 hand theirs to wave 0
// dQ_of(j): the caller's slot sum of position j's dQs.  True for the lanes that hold the block's pU / pCq / pC2 (wave 0,
// c < w): they write the caller's row of parameter-vector partials.
template <class DQ>
__device__ __forceinline__ bool attn_bwd_fold_body(const float* __restrict__ vecs, const float* __restrict__ hq,
                                                   float* __restrict__ d_hq, bool acc_hq, const float* __restrict__ dctp,
                                                   size_t dct_stride, int nslot, float* __restrict__ dctn, int w, int JP,
                                                   int JQ, DQ dQ_of, f32x4& pU, f32x4& pCq, f32x4& pC2) {
  __shared__ float s_dct[64];
  __shared__ f32x4 s_p[3][3][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = blockIdx.y * 256 + 4 * lane;
  if (tid < JP) {
    const float dct = attn_bwd_slot_sum<float>(nslot, [&](int i) { return dctp[(size_t)i * dct_stride + tid]; });
    s_dct[tid] = dct;
    if (blockIdx.y == 0 && blockIdx.z == 0) dctn[tid] = dct;
  }
  __syncthreads();
  const bool live = c < w;
  const f32x4 U = ld4_if(live, vecs + VEC_U * w + c), Cq = ld4_if(live, vecs + VEC_CQ * w + c),
              C2 = ld4_if(live, vecs + VEC_C2 * w + c);
  pU = pCq = pC2 = zero4();
  const int j_lo = blockIdx.z * ATTN_BWD_JG, j_hi = min(JQ, j_lo + ATTN_BWD_JG);
  for (int j = j_lo + wave; j < j_hi; j += 4) {
    const f32x4 dQ = dQ_of(j);
    const f32x4 qv = ld4_if(live, hq + (size_t)j * w + c);
    const float dct = s_dct[j];
    const f32x4 dq = U * dQ + dct * (Cq + 2.f * C2 * qv);
    if (live) {
      f32x4* dst = reinterpret_cast<f32x4*>(d_hq + (size_t)j * w + c);
      *dst = acc_hq ? *dst + dq : dq;
    }
    pU += dQ * qv;
    pCq += dct * qv;
    pC2 += dct * qv * qv;
  }
  if (wave) {
    s_p[wave - 1][0][lane] = pU;
    s_p[wave - 1][1][lane] = pCq;
    s_p[wave - 1][2][lane] = pC2;
  }
  __syncthreads();
  if (wave || !live) return false;
#pragma unroll
  for (int v = 0; v < 3; ++v) {  // wave order: positions j_lo + v (+ 4) after j_lo (+ 4)
    pU += s_p[v][0][lane];
    pCq += s_p[v][1][lane];
    pC2 += s_p[v][2][lane];
  }
  return true;
}

// ---- the parameter kernels: grid ceil(w / 64) + 1; 256 threads = 64 channels x 4 thread groups that stride over the rows
// of partials; the last block is the bias block.  Fixed summation order throughout.
// the bias block: db += the sum of the `count` d ct values (db null: nothing)
__device__ __forceinline__ void attn_bwd_bias_block(const float* __restrict__ dctn, size_t count, float* __restrict__ db) {
  __shared__ float s_b[4];
  const int tid = threadIdx.x;
  float acc = 0.f;
  for (size_t i = tid; i < count; i += 256) acc += dctn[i];
  acc = wave_sum(acc);
  if ((tid & 63) == 0) s_b[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0 && db) db[0] += (s_b[0] + s_b[1]) + (s_b[2] + s_b[3]);
}

// thread group `part` of channel c: vector `which` of the rows part, part + 4, ... of base [rows][per][w], added in that
// order, eight rows in flight
__device__ __forceinline__ float attn_bwd_sum_rows(const float* __restrict__ base, size_t rows, int per, int which, int part,
                                                   int w, int c) {
  float acc = 0.f;
  size_t i = part;
  for (; i + 28 < rows; i += 32) {
    float x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = base[((i + 4 * u) * per + which) * w + c];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += x[u];
  }
  for (; i < rows; i += 4) acc += base[(i * per + which) * w + c];
  return acc;
}

// the four groups' sums of channel c, (g0 + g1) + (g2 + g3), into dW (attn_common.h's mapping)
__device__ __forceinline__ void attn_bwd_combine_dW(const float (&v)[VEC_COUNT], int simi, int feat_order, int w, int c,
                                                    float* __restrict__ dW) {
  __shared__ float s_p[4][VEC_COUNT][64];
  const int cl = threadIdx.x & 63, part = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < VEC_COUNT; ++k) s_p[part][k][cl] = v[k];
  __syncthreads();
  if (part == 0 && c < w) {
    float t[VEC_COUNT];
#pragma unroll
    for (int k = 0; k < VEC_COUNT; ++k) t[k] = (s_p[0][k][cl] + s_p[1][k][cl]) + (s_p[2][k][cl] + s_p[3][k][cl]);
    attn_bwd_add_dW(simi, feat_order, w, c, t[VEC_U], t[VEC_RH], t[VEC_R2], t[VEC_CQ], t[VEC_C2], dW);
  }
}

// ---- sum of one double per thread over a workgroup of 256 (a tree in LDS); the result is thread 0's
__device__ __forceinline__ double attn_bwd_block_sum_f64(double acc) {
  __shared__ double s_acc[256];
  s_acc[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s_acc[threadIdx.x] += s_acc[threadIdx.x + o];
    __syncthreads();
  }
  return s_acc[0];
}

// ---- the dense logit-gradient paths (attn_dense.hip: K = 1 rows resident in LDS, where the kernel is; attn_cube_bwd.hip: any
// K, tiled over T): fold the per-n partials pvec [N][5][w], pb [N] in n order into dW and db.  grid ceil(w/256) + 1
__global__ __launch_bounds__(256) void attn_logits_bwd_params_kernel(const float* __restrict__ pvec, const float* __restrict__ pb,
                                                                    float* __restrict__ dW, float* __restrict__ db, int N, int w,
                                                                    int simi, int feat_order);

}  // namespace fvta
