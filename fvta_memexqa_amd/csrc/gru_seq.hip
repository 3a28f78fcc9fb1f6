// A GRU over a whole sequence, forward and backward, for gfx950: TensorFlow 1's GRUCell under dynamic_rnn(sequence_length)
// (the cell of model_dmnplus.py:344-345, 470-471; the formulas are those of include/fvta_hip.h, unpinned):
//   [r | u] = sigmoid([x_t, h] Wg + bg)     c = tanh([x_t, r * h] Wc + bc)     h' = u * h + (1 - u) * c
// Row n takes lens[n] steps; after them its state is carried and its output rows are zero.  reverse = 1 walks row n from
// lens[n] - 1 down to 0 (the backward half of bidirectional_dynamic_rnn) by indexing: step s of row n is position
// lens[n] - 1 - s while s < lens[n], and position s (a padded one) from then on.
// What does not depend on the state is hoisted out of the recurrence, as in attgru_seq.hip: x Wg[:in] + bg and
// x Wc[:in] + bc for all N*T rows before it (fvta_linear_fwd), and d_x and the four parameter gradients as contractions over
// all N*T rows after the reverse recurrence (fvta_linear_bwd over the gate gradients it leaves in the workspace; those of
// a padded step are zero, so the contractions take no mask).
// The recurrence is TWO dependent products per step -- h Wg[in:] gives r and u, (r * h) Wc[in:] gives c -- and a workgroup
// owns SEQ_RT = 16 rows, so no workgroup ever waits for another.  Two regimes, by d:
//   A (dp = d rounded up to 16 <= 128): ONE launch for all T steps, dp / 16 waves.  A wave owns 16 units and keeps their
//     r, u and c columns of the state-side weights in REGISTERS as MFMA B fragments (3 dp / 4 per lane); LDS holds only the
//     state tile and the r * h tile, [16][dp + 2] each.  Two barriers per step, reached by every wave.
//   B (larger d): a step is two fused launches over (row tiles x 64-unit column tiles), one per product, the gate math as
//     epilogue.  Issued from one C call, ordered by the stream.
// No atomics, fixed summation order: two runs are bitwise equal.  The backward only reads `saved`.
#include "seq_common.h"

namespace fvta {

// Register budget of regime A: a SIMD has 512 registers per lane; at two waves per SIMD a wave may use 256.  The weight
// fragments take 3 dp / 4 of them, the rest of a step (accumulators, gate inputs, addresses, the state) fits in 96.
constexpr int GRU_A_REGS_PER_WAVE = 512 / (SEQ_A_WAVES / 4);   // (SEQ_A_WAVES = 8, 512 threads: two waves per SIMD)
constexpr int GRU_A_REGS_OTHER = 96;
static_assert(3 * SEQ_A_DP_MAX / 4 + GRU_A_REGS_OTHER <= GRU_A_REGS_PER_WAVE, "regime A's weight fragments must fit the registers");
static_assert(4 * SEQ_RT * (SEQ_A_DP_MAX + 2) * 4 <= 64 * 1024, "regime A's tiles must fit static LDS");

struct GruFwdArgs {
  int N, T, in, d, reverse;
  const int* lens;
  const float *h0, *Wg, *Wc, *preG, *preC;
  float *out, *h_last, *S_h, *S_r, *S_u, *S_c;
};
struct GruBwdArgs {
  int N, T, in, d, reverse;
  const int* lens;
  const float *Wg, *Wc, *S_h, *S_r, *S_u, *S_c, *d_out, *d_h_last;
  float *G_g, *G_c, *RH, *d_h0;
};

// the position step s of a row of length len works on
__device__ __forceinline__ int gru_pos(int s, int len, int reverse) { return (reverse && s < len) ? len - 1 - s : s; }
__device__ __forceinline__ int gru_len(const int* lens, int n, int T) {
  if (!lens) return T;
  const int l = lens[n];
  return l < 0 ? 0 : (l > T ? T : l);
}

// The state update (the fmaf: see "Rounding" in seq_common.h)
__device__ __forceinline__ float gru_update(float u, float h, float c) { return fmaf(u, h, (1.f - u) * c); }

// gate gradients of one element from dt = d(h'): returns the part of d(h) that does not pass through a product
__device__ __forceinline__ float gru_gate_bwd(float dt, float hp, float u, float c, float& dc_pre, float& du_pre) {
  dc_pre = dt * (1.f - u) * (1.f - c * c);
  du_pre = dt * (hp - c) * u * (1.f - u);
  return dt * u;
}

// ---------------------------------------------------------------- regime A
// These two kernels keep their lane preamble, h0 load and row stores written out: with any of seq_common.h's helpers in
// them the compiler schedules the register-tight step loop differently (measured: 0.2-0.4 % slower at d = 100).
// grid ceil(N/16), 64 KT threads; KT = dp / 16
template <int KT, bool TRAIN>
__global__ __launch_bounds__(64 * KT) void gru_seq_fwd_a(GruFwdArgs a) {
  constexpr int DP = 16 * KT, LD = DP + 2, NK = DP / 4;
  __shared__ float H_l[SEQ_RT * LD], RH_l[SEQ_RT * LD];   // h_{t-1} and r * h_{t-1} of the tile: the A operands
  const int N = a.N, T = a.T, d = a.d;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int m0 = blockIdx.x * SEQ_RT;
  const int u = wave * 16 + (lane & 15), kq = lane >> 4, i0 = 4 * kq;
  const float* Wgs = a.Wg + (size_t)a.in * 2 * d;   // [d][2d]: the state rows
  const float* Wcs = a.Wc + (size_t)a.in * d;       // [d][d]
  float wr[NK], wu[NK], wc[NK];                     // B fragments: W[k = 4 j + kq][u]
#pragma unroll
  for (int j = 0; j < NK; ++j) {
    const int k = 4 * j + kq;
    const bool ok = k < d && u < d;
    const size_t k_ = ok ? k : 0, u_ = ok ? u : 0;
    const float vr = Wgs[k_ * 2 * d + u_], vu = Wgs[k_ * 2 * d + d + u_], vc = Wcs[k_ * d + u_];
    wr[j] = ok ? vr : 0.f;
    wu[j] = ok ? vu : 0.f;
    wc[j] = ok ? vc : 0.f;
  }
  for (int idx = tid; idx < SEQ_RT * DP; idx += 64 * KT) {
    const int i = idx / DP, c = idx - i * DP, n = m0 + i;
    float v = 0.f;
    if (a.h0 && n < N && c < d) v = a.h0[(size_t)n * d + c];
    H_l[i * LD + c] = v;
  }
  __syncthreads();
  float h[4];
  bool ok[4];
  int len[4];
  int64_t row[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = m0 + i0 + r;
    ok[r] = n < N && u < d;
    row[r] = n < N ? n : 0;
    len[r] = ok[r] ? gru_len(a.lens, (int)row[r], T) : 0;
    h[r] = H_l[(i0 + r) * LD + u];
  }
  const float* ha = H_l + (lane & 15) * LD + kq;
  const float* rha = RH_l + (lane & 15) * LD + kq;
  for (int s = 0; s < T; ++s) {
    float pr[4], pu[4], pc[4];
    int64_t sidx[4];
    bool valid[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {   // (state independent: issued ahead of the products)
      const int64_t rt = row[r] * T + gru_pos(s, len[r], a.reverse);
      valid[r] = s < len[r];        // (len is 0 off the tensor)
      sidx[r] = ok[r] ? rt * d + u : 0;
      const int64_t g = ok[r] ? rt * 2 * d + u : 0;
      pr[r] = a.preG[g];
      pu[r] = a.preG[ok[r] ? g + d : 0];
      pc[r] = a.preC[sidx[r]];
    }
    f32x4 acc_r = zero4(), acc_u = zero4(), acc_c = zero4();
#pragma unroll
    for (int j = 0; j < NK; ++j) {
      const float av = ha[4 * j];
      acc_r = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wr[j], acc_r, 0, 0, 0);
      acc_u = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wu[j], acc_u, 0, 0, 0);
    }
    float rr[4], uu[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      rr[r] = fvta_sigmoid(acc_r[r] + pr[r]);
      uu[r] = fvta_sigmoid(acc_u[r] + pu[r]);
      RH_l[(i0 + r) * LD + u] = rr[r] * h[r];     // (h is 0 off the tensor)
    }
    __syncthreads();                // every wave has read H_l and written its columns of RH_l
#pragma unroll
    for (int j = 0; j < NK; ++j) acc_c = __builtin_amdgcn_mfma_f32_16x16x4f32(rha[4 * j], wc[j], acc_c, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float cc = fvta_tanh(acc_c[r] + pc[r]);
      const float hn = gru_update(uu[r], h[r], cc);
      if (ok[r]) {
        if (TRAIN) {
          a.S_h[sidx[r]] = valid[r] ? h[r] : 0.f;   // (a finite value on padded steps: the contractions read it)
          a.S_r[sidx[r]] = rr[r];
          a.S_u[sidx[r]] = uu[r];
          a.S_c[sidx[r]] = cc;
        }
        if (a.out) a.out[sidx[r]] = valid[r] ? hn : 0.f;
      }
      h[r] = valid[r] ? hn : h[r];
      H_l[(i0 + r) * LD + u] = h[r];
    }
    __syncthreads();                // every wave has read RH_l and written its columns of H_l
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (ok[r]) a.h_last[row[r] * d + u] = h[r];
}

// grid ceil(N/16), 64 KT threads.  A wave owns 16 units k of d(h): its fragments are rows k of the state-side weights.
template <int KT>
__global__ __launch_bounds__(64 * KT) void gru_seq_bwd_a(GruBwdArgs a) {
  constexpr int DP = 16 * KT, LD = DP + 2, NK = DP / 4;
  __shared__ float Tc[SEQ_RT * LD], Tr[SEQ_RT * LD], Tu[2][SEQ_RT * LD];   // dc_pre, dr_pre, du_pre of the step
  const int N = a.N, T = a.T, d = a.d;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int m0 = blockIdx.x * SEQ_RT;
  const int u = wave * 16 + (lane & 15), kq = lane >> 4, i0 = 4 * kq;
  const float* Wgs = a.Wg + (size_t)a.in * 2 * d;
  const float* Wcs = a.Wc + (size_t)a.in * d;
  float wr[NK], wu[NK], wc[NK];                     // B fragments: W[u][j = 4 jj + kq] (the transposed product)
#pragma unroll
  for (int jj = 0; jj < NK; ++jj) {
    const int j = 4 * jj + kq;
    const bool ok = j < d && u < d;
    const size_t j_ = ok ? j : 0, u_ = ok ? u : 0;
    const float vr = Wgs[u_ * 2 * d + j_], vu = Wgs[u_ * 2 * d + d + j_], vc = Wcs[u_ * d + j_];
    wr[jj] = ok ? vr : 0.f;
    wu[jj] = ok ? vu : 0.f;
    wc[jj] = ok ? vc : 0.f;
  }
  float dh[4];
  bool ok[4];
  int len[4];
  int64_t row[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = m0 + i0 + r;
    ok[r] = n < N && u < d;
    row[r] = n < N ? n : 0;
    len[r] = ok[r] ? gru_len(a.lens, (int)row[r], T) : 0;
    dh[r] = (ok[r] && a.d_h_last) ? a.d_h_last[row[r] * d + u] : 0.f;
  }
  const int ao = (lane & 15) * LD + kq;
  for (int s = T - 1; s >= 0; --s) {
    float* Tu_s = Tu[s & 1];        // (double buffered: the next step writes it while a slow wave still reads this one)
    float hp[4], rr[4], keep[4];
    int64_t sidx[4], gidx[4];
    bool valid[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t rt = row[r] * T + gru_pos(s, len[r], a.reverse);
      valid[r] = s < len[r];
      sidx[r] = ok[r] ? rt * d + u : 0;
      gidx[r] = ok[r] ? rt * 2 * d + u : 0;
      float dc_pre = 0.f, du_pre = 0.f;
      hp[r] = rr[r] = 0.f;
      keep[r] = dh[r];
      if (valid[r]) {
        hp[r] = a.S_h[sidx[r]];
        rr[r] = a.S_r[sidx[r]];
        const float dt = dh[r] + (a.d_out ? a.d_out[sidx[r]] : 0.f);
        keep[r] = gru_gate_bwd(dt, hp[r], a.S_u[sidx[r]], a.S_c[sidx[r]], dc_pre, du_pre);
      }
      Tc[(i0 + r) * LD + u] = dc_pre;
      Tu_s[(i0 + r) * LD + u] = du_pre;
      if (ok[r]) {
        a.G_c[sidx[r]] = dc_pre;
        a.G_g[gidx[r] + d] = du_pre;
        a.RH[sidx[r]] = rr[r] * hp[r];
      }
    }
    __syncthreads();
    f32x4 acc = zero4();            // d(r * h) = dc_pre Wc[in:]^T
#pragma unroll
    for (int jj = 0; jj < NK; ++jj) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Tc[ao + 4 * jj], wc[jj], acc, 0, 0, 0);
    f32x4 acc0, acc1 = zero4();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float dr_pre = acc[r] * hp[r] * rr[r] * (1.f - rr[r]);   // (hp = rr = 0 on a padded step)
      Tr[(i0 + r) * LD + u] = dr_pre;
      if (ok[r]) a.G_g[gidx[r]] = dr_pre;
      acc0[r] = fmaf(acc[r], rr[r], keep[r]);
    }
    __syncthreads();
#pragma unroll
    for (int jj = 0; jj < NK; ++jj) {   // + [dr_pre | du_pre] Wg[in:]^T
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(Tr[ao + 4 * jj], wr[jj], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(Tu_s[ao + 4 * jj], wu[jj], acc1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) dh[r] = ok[r] ? acc0[r] + acc1[r] : 0.f;
  }
  if (a.d_h0)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (ok[r]) a.d_h0[row[r] * d + u] = dh[r];
}

// ---------------------------------------------------------------- regime B
// Step s, product 1.  grid (ceil(N/16), ceil(d/64)), 256 threads.  h_prev [N,d] (NULL: zeros) -> rh = r * h_prev, ub = u
template <bool TRAIN>
__global__ __launch_bounds__(256) void gru_seq_fwd_b1(GruFwdArgs a, int s, const float* __restrict__ h_prev,
                                                      float* __restrict__ rh, float* __restrict__ ub) {
  __shared__ float A_l[SEQ_RT * SEQ_B_LD], Br_l[SEQ_B_CT * SEQ_B_LD], Bu_l[SEQ_B_CT * SEQ_B_LD];
  const int N = a.N, T = a.T, d = a.d;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int m0 = blockIdx.x * SEQ_RT, c0 = blockIdx.y * SEQ_B_CT;
  const float* Wgs = a.Wg + (size_t)a.in * 2 * d;
  f32x4 acc_r = zero4(), acc_u = zero4();
  for (int k0 = 0; k0 < d; k0 += SEQ_B_KC) {
    seq_stage_a(A_l, h_prev, d, N, d, m0, k0, tid);
    seq_stage_w2<false>(Br_l, Bu_l, Wgs, Wgs + d, (size_t)2 * d, d, c0, k0, tid);
    __syncthreads();
    seq_mma2(A_l, SEQ_B_LD, Br_l + wave * 16 * SEQ_B_LD, Bu_l + wave * 16 * SEQ_B_LD, SEQ_B_LD, SEQ_B_KC, lane, acc_r, acc_u);
    __syncthreads();
  }
  const auto [u, i0] = seq_lane(wave, lane, c0);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = m0 + i0 + r;
    if (seq_live(n, u, N, d)) {
      const int len = gru_len(a.lens, n, T);
      const int64_t rt = (int64_t)n * T + gru_pos(s, len, a.reverse);
      const float hp = h_prev ? h_prev[(int64_t)n * d + u] : 0.f;
      const float rr = fvta_sigmoid(acc_r[r] + a.preG[rt * 2 * d + u]);
      const float uu = fvta_sigmoid(acc_u[r] + a.preG[rt * 2 * d + d + u]);
      rh[(int64_t)n * d + u] = rr * hp;
      ub[(int64_t)n * d + u] = uu;
      if (TRAIN) {
        a.S_h[rt * d + u] = s < len ? hp : 0.f;
        a.S_r[rt * d + u] = rr;
        a.S_u[rt * d + u] = uu;
      }
    }
  }
}

// Step s, product 2.  grid as above.  h_new may be h_prev: a thread reads its own element of h_prev only.
template <bool TRAIN>
__global__ __launch_bounds__(256) void gru_seq_fwd_b2(GruFwdArgs a, int s, const float* h_prev, const float* __restrict__ rh,
                                                      const float* __restrict__ ub, float* h_new) {
  __shared__ float A_l[SEQ_RT * SEQ_B_LD], Bc_l[SEQ_B_CT * SEQ_B_LD];
  const int N = a.N, T = a.T, d = a.d;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int m0 = blockIdx.x * SEQ_RT, c0 = blockIdx.y * SEQ_B_CT;
  const float* Wcs = a.Wc + (size_t)a.in * d;
  f32x4 acc = zero4();
  for (int k0 = 0; k0 < d; k0 += SEQ_B_KC) {
    seq_stage_a(A_l, rh, d, N, d, m0, k0, tid);
    seq_stage_w1<false>(Bc_l, Wcs, d, d, c0, k0, tid);
    __syncthreads();
    seq_mma1(A_l, SEQ_B_LD, Bc_l + wave * 16 * SEQ_B_LD, SEQ_B_LD, SEQ_B_KC, lane, acc);
    __syncthreads();
  }
  const auto [u, i0] = seq_lane(wave, lane, c0);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = m0 + i0 + r;
    if (seq_live(n, u, N, d)) {
      const int len = gru_len(a.lens, n, T);
      const int64_t sidx = ((int64_t)n * T + gru_pos(s, len, a.reverse)) * d + u;
      const bool valid = s < len;
      const float hp = h_prev ? h_prev[(int64_t)n * d + u] : 0.f;
      const float cc = fvta_tanh(acc[r] + a.preC[sidx]);
      const float hn = gru_update(ub[(int64_t)n * d + u], hp, cc);
      if (TRAIN) a.S_c[sidx] = cc;
      if (a.out) a.out[sidx] = valid ? hn : 0.f;
      h_new[(int64_t)n * d + u] = valid ? hn : hp;
    }
  }
}

// Reverse step s, product 1: d(r * h) = dc_pre Wc[in:]^T, then every gate gradient of the step.  grid as above.
// d_cur [N,d] (NULL: zeros) is d(h') carried from the later steps; dhp gets d(h) without the second product's share.
__global__ __launch_bounds__(256) void gru_seq_bwd_b1(GruBwdArgs a, int s, const float* __restrict__ d_cur,
                                                      float* __restrict__ dhp) {
  __shared__ float Tc[SEQ_RT * SEQ_B_LD], Bc_l[SEQ_B_CT * SEQ_B_LD];
  const int N = a.N, T = a.T, d = a.d;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int m0 = blockIdx.x * SEQ_RT, c0 = blockIdx.y * SEQ_B_CT;
  const float* Wcs = a.Wc + (size_t)a.in * d;
  f32x4 acc = zero4();
  for (int k0 = 0; k0 < d; k0 += SEQ_B_KC) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {   // the A operand: dc_pre of (n, j), recomputed by every column tile
      int i, kk;
      seq_b_decode(tid, p, i, kk);
      const int n = m0 + i, j = k0 + kk;
      float dc_pre = 0.f, du_pre;
      if (n < N && j < d) {
        const int len = gru_len(a.lens, n, T);
        if (s < len) {
          const int64_t sidx = ((int64_t)n * T + gru_pos(s, len, a.reverse)) * d + j;
          const float dt = (d_cur ? d_cur[(int64_t)n * d + j] : 0.f) + (a.d_out ? a.d_out[sidx] : 0.f);
          (void)gru_gate_bwd(dt, 0.f, a.S_u[sidx], a.S_c[sidx], dc_pre, du_pre);
        }
      }
      Tc[i * SEQ_B_LD + kk] = dc_pre;
    }
    seq_stage_w1<true>(Bc_l, Wcs, d, d, c0, k0, tid);
    __syncthreads();
    seq_mma1(Tc, SEQ_B_LD, Bc_l + wave * 16 * SEQ_B_LD, SEQ_B_LD, SEQ_B_KC, lane, acc);
    __syncthreads();
  }
  const auto [u, i0] = seq_lane(wave, lane, c0);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = m0 + i0 + r;
    if (seq_live(n, u, N, d)) {
      const int len = gru_len(a.lens, n, T);
      const int64_t rt = (int64_t)n * T + gru_pos(s, len, a.reverse), sidx = rt * d + u;
      const float dc = d_cur ? d_cur[(int64_t)n * d + u] : 0.f;
      float dc_pre = 0.f, du_pre = 0.f, dr_pre = 0.f, rhv = 0.f, keep = dc;
      if (s < len) {
        const float hp = a.S_h[sidx], rr = a.S_r[sidx];
        const float dt = dc + (a.d_out ? a.d_out[sidx] : 0.f);
        keep = fmaf(acc[r], rr, gru_gate_bwd(dt, hp, a.S_u[sidx], a.S_c[sidx], dc_pre, du_pre));
        dr_pre = acc[r] * hp * rr * (1.f - rr);
        rhv = rr * hp;
      }
      a.G_g[rt * 2 * d + u] = dr_pre;
      a.G_g[rt * 2 * d + d + u] = du_pre;
      a.G_c[sidx] = dc_pre;
      a.RH[sidx] = rhv;
      dhp[(int64_t)n * d + u] = keep;
    }
  }
}

// Reverse step s, product 2: d_next = dhp + [dr_pre | du_pre] Wg[in:]^T, the gate gradients read back from the workspace.
__global__ __launch_bounds__(256) void gru_seq_bwd_b2(GruBwdArgs a, int s, const float* __restrict__ dhp,
                                                      float* __restrict__ d_next) {
  __shared__ float Tr[SEQ_RT * SEQ_B_LD], Tu[SEQ_RT * SEQ_B_LD], Br_l[SEQ_B_CT * SEQ_B_LD], Bu_l[SEQ_B_CT * SEQ_B_LD];
  const int N = a.N, T = a.T, d = a.d;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int m0 = blockIdx.x * SEQ_RT, c0 = blockIdx.y * SEQ_B_CT;
  const float* Wgs = a.Wg + (size_t)a.in * 2 * d;
  f32x4 acc0 = zero4(), acc1 = zero4();
  for (int k0 = 0; k0 < d; k0 += SEQ_B_KC) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      int i, kk;
      seq_b_decode(tid, p, i, kk);
      const int n = m0 + i, j = k0 + kk;
      float vr = 0.f, vu = 0.f;
      if (n < N && j < d) {
        const int64_t g = ((int64_t)n * T + gru_pos(s, gru_len(a.lens, n, T), a.reverse)) * 2 * d + j;
        vr = a.G_g[g];
        vu = a.G_g[g + d];
      }
      Tr[i * SEQ_B_LD + kk] = vr;
      Tu[i * SEQ_B_LD + kk] = vu;
    }
    seq_stage_w2<true>(Br_l, Bu_l, Wgs, Wgs + d, (size_t)2 * d, d, c0, k0, tid);
    __syncthreads();
    seq_mma_ab(Tr, Tu, SEQ_B_LD, Br_l + wave * 16 * SEQ_B_LD, Bu_l + wave * 16 * SEQ_B_LD, SEQ_B_LD, SEQ_B_KC, lane, acc0, acc1);
    __syncthreads();
  }
  const auto [u, i0] = seq_lane(wave, lane, c0);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = m0 + i0 + r;
    if (seq_live(n, u, N, d)) d_next[(int64_t)n * d + u] = dhp[(int64_t)n * d + u] + (acc0[r] + acc1[r]);
  }
}

static inline size_t gru_n(const fvta_gru_seq_desc& d) { return (size_t)d.N * d.T * d.d; }
// saved: h_{t-1}, r, u, c.  workspace, forward: the hoisted products x Wg[:in] + bg (a, 2 n) and x Wc[:in] + bc (b), r * h and
// u of a step (s0, s1: regime B); backward: the gate gradients [dr | du] (a) and dc (b), r * h of every step (c), two d_h rows
static inline SeqWork gru_work(const fvta_gru_seq_desc& d, int backward, void* p) {
  return SeqWork(gru_n(d), (size_t)d.N * d.d, 2, backward != 0, p);
}

static inline bool gru_desc_ok(const fvta_gru_seq_desc* d) {
  return d && d->N > 0 && d->T > 0 && d->in_dim > 0 && d->d > 0 && (d->reverse == 0 || d->reverse == 1);
}

template <int KT>
static void gru_launch_fwd_a(const GruFwdArgs& a, bool training, unsigned row_tiles, hipStream_t s) {
  if (training) hipLaunchKernelGGL((gru_seq_fwd_a<KT, true>), dim3(row_tiles), dim3(64 * KT), 0, s, a);
  else hipLaunchKernelGGL((gru_seq_fwd_a<KT, false>), dim3(row_tiles), dim3(64 * KT), 0, s, a);
}
template <int KT>
static void gru_launch_bwd_a(const GruBwdArgs& a, unsigned row_tiles, hipStream_t s) {
  hipLaunchKernelGGL((gru_seq_bwd_a<KT>), dim3(row_tiles), dim3(64 * KT), 0, s, a);
}

}  // namespace fvta
using namespace fvta;

#define GRU_A_DISPATCH(kt, CALL)    \
  switch (kt) {                     \
    case 1: CALL(1); break;         \
    case 2: CALL(2); break;         \
    case 3: CALL(3); break;         \
    case 4: CALL(4); break;         \
    case 5: CALL(5); break;         \
    case 6: CALL(6); break;         \
    case 7: CALL(7); break;         \
    default: CALL(8); break;        \
  }

extern "C" size_t fvta_gru_seq_saved_bytes(const fvta_gru_seq_desc* d) {
  if (!gru_desc_ok(d)) return seq_refuse("gru_seq_saved_bytes: bad N/T/in_dim/d/reverse");
  return d->training ? SeqSaved(gru_n(*d), nullptr).bytes : 0;
}

extern "C" size_t fvta_gru_seq_workspace_bytes(const fvta_gru_seq_desc* d, int32_t backward) {
  if (!gru_desc_ok(d)) return seq_refuse("gru_seq_workspace_bytes: bad N/T/in_dim/d/reverse");
  return gru_work(*d, backward, nullptr).bytes;
}

extern "C" int fvta_gru_seq_plan(const fvta_gru_seq_desc* d, int32_t* out) {
  FVTA_CHECK_ARG(gru_desc_ok(d), "gru_seq_plan: bad N/T/in_dim/d/reverse");
  FVTA_CHECK_ARG(out, "gru_seq_plan: null pointer");
  seq_fill_plan(out, seq_regime_a(d->d), 2, d->T);
  return FVTA_OK;
}

extern "C" int fvta_gru_seq_fwd(const fvta_gru_seq_desc* d, const float* x, const int32_t* lens, const float* h0,
                                const float* Wg, const float* bg, const float* Wc, const float* bc, float* out, float* h_last,
                                void* saved, void* workspace, fvta_stream_t stream_) {
  FVTA_CHECK_ARG(gru_desc_ok(d), "gru_seq_fwd: bad N/T/in_dim/d/reverse");
  FVTA_CHECK_ARG(x && Wg && bg && Wc && bc && h_last && workspace, "gru_seq_fwd: null pointer");
  FVTA_CHECK_ARG(!d->training || saved, "gru_seq_fwd: training wants `saved`");
  hipStream_t s = (hipStream_t)stream_;
  const int N = d->N, T = d->T, in = d->in_dim, dd = d->d;
  const SeqWork w = gru_work(*d, 0, workspace);
  const SeqSaved sv(gru_n(*d), d->training ? saved : nullptr);
  const int64_t M = (int64_t)N * T;
  int st = fvta_linear_fwd(x, Wg, bg, w.a, M, in, 2 * dd, 0, stream_);   // x Wg[:in] + bg
  if (st != FVTA_OK) return st;
  st = fvta_linear_fwd(x, Wc, bc, w.b, M, in, dd, 0, stream_);           // x Wc[:in] + bc
  if (st != FVTA_OK) return st;
  GruFwdArgs a{N, T, in, dd, d->reverse, lens, h0, Wg, Wc, w.a, w.b, out, h_last, sv.s[0], sv.s[1], sv.s[2], sv.s[3]};
  const unsigned row_tiles = seq_row_tiles(N);
  if (seq_regime_a(dd)) {
    const bool tr = d->training != 0;
#define GRU_CALL(KT) gru_launch_fwd_a<KT>(a, tr, row_tiles, s)
    GRU_A_DISPATCH(seq_dp(dd) / 16, GRU_CALL)
#undef GRU_CALL
  } else {
    const dim3 grid = seq_grid_b(N, dd);
    for (int t = 0; t < T; ++t) {   // the state lives in h_last from the first step on
      const float* hp = t == 0 ? h0 : h_last;
      if (d->training) {
        hipLaunchKernelGGL(gru_seq_fwd_b1<true>, grid, dim3(256), 0, s, a, t, hp, w.s0, w.s1);
        hipLaunchKernelGGL(gru_seq_fwd_b2<true>, grid, dim3(256), 0, s, a, t, hp, w.s0, w.s1, h_last);
      } else {
        hipLaunchKernelGGL(gru_seq_fwd_b1<false>, grid, dim3(256), 0, s, a, t, hp, w.s0, w.s1);
        hipLaunchKernelGGL(gru_seq_fwd_b2<false>, grid, dim3(256), 0, s, a, t, hp, w.s0, w.s1, h_last);
      }
    }
  }
  FVTA_CHECK_LAUNCH("gru_seq_fwd");
  return FVTA_OK;
}

extern "C" int fvta_gru_seq_bwd(const fvta_gru_seq_desc* d, const float* x, const int32_t* lens, const float* Wg,
                                const float* Wc, const void* saved, const float* d_out, const float* d_h_last, float* d_x,
                                float* d_h0, float* dWg, float* dbg, float* dWc, float* dbc, int32_t accumulate,
                                void* workspace, fvta_stream_t stream_) {
  FVTA_CHECK_ARG(gru_desc_ok(d), "gru_seq_bwd: bad N/T/in_dim/d/reverse");
  FVTA_CHECK_ARG(d->training, "gru_seq_bwd: the forward ran with training = 0, nothing was saved");
  FVTA_CHECK_ARG(x && Wg && Wc && saved && d_x && dWg && dbg && dWc && dbc && workspace, "gru_seq_bwd: null pointer");
  FVTA_CHECK_ARG(d_out || d_h_last, "gru_seq_bwd: d_out and d_h_last are both NULL");
  hipStream_t s = (hipStream_t)stream_;
  const int N = d->N, T = d->T, in = d->in_dim, dd = d->d;
  const SeqWork w = gru_work(*d, 1, workspace);
  const SeqSaved sv(gru_n(*d), const_cast<void*>(saved));
  if (!accumulate)
    seq_zero_params({{dWg, dWc, dbg, dbc}, {(int64_t)(in + dd) * 2 * dd, (int64_t)(in + dd) * dd, 2 * dd, dd}}, s);
  GruBwdArgs a{N, T, in, dd, d->reverse, lens, Wg, Wc, sv.s[0], sv.s[1], sv.s[2], sv.s[3], d_out, d_h_last, w.a, w.b, w.c, d_h0};
  const unsigned row_tiles = seq_row_tiles(N);
  if (seq_regime_a(dd)) {
#define GRU_CALL(KT) gru_launch_bwd_a<KT>(a, row_tiles, s)
    GRU_A_DISPATCH(seq_dp(dd) / 16, GRU_CALL)
#undef GRU_CALL
  } else {
    const dim3 grid = seq_grid_b(N, dd);
    const float* cur = d_h_last;
    for (int t = T - 1; t >= 0; --t) {
      float* nxt = (t == 0 && d_h0) ? d_h0 : w.s0;
      hipLaunchKernelGGL(gru_seq_bwd_b1, grid, dim3(256), 0, s, a, t, cur, w.s1);
      hipLaunchKernelGGL(gru_seq_bwd_b2, grid, dim3(256), 0, s, a, t, w.s1, nxt);
      cur = nxt;
    }
  }
  FVTA_CHECK_LAUNCH("gru_seq_bwd");
  // contractions over all N*T rows: d_x = [dr|du] Wg[:in]^T + dc Wc[:in]^T; dWg[:in], dbg, dWc[:in], dbc from x;
  // dWg[in:] from h_{t-1}, dWc[in:] from r * h_{t-1}
  const int64_t M = (int64_t)N * T;
  const size_t og = (size_t)in * 2 * dd, oc = (size_t)in * dd;
  int st = fvta_linear_bwd(x, Wg, nullptr, w.a, d_x, dWg, dbg, M, in, 2 * dd, 0, 0, stream_);
  if (st != FVTA_OK) return st;
  st = fvta_linear_bwd(x, Wc, nullptr, w.b, d_x, dWc, dbc, M, in, dd, 0, 1, stream_);
  if (st != FVTA_OK) return st;
  st = fvta_linear_bwd(sv.s[0], Wg + og, nullptr, w.a, nullptr, dWg + og, nullptr, M, dd, 2 * dd, 0, 0, stream_);
  if (st != FVTA_OK) return st;
  return fvta_linear_bwd(w.c, Wc + oc, nullptr, w.b, nullptr, dWc + oc, nullptr, M, dd, dd, 0, 0, stream_);
}
