// The AttentionGRU over a whole fact sequence (model_dmnplus.py:123-134: dynamic_rnn over AttentionGRUCell,
// attention_gru_cell.py:50-70), forward and backward, for gfx950:
//   r_t  = sigmoid(x_t Wg[:d] + h_{t-1} Wg[d:] + bg)     hc_t = h_{t-1} Wc     xi_t = x_t Wi + bi
//   hh_t = tanh(r_t * hc_t + xi_t)                        h_t  = (1 - g_t) h_{t-1} + g_t hh_t
// What does not depend on the state is hoisted out of the recurrence: pre = [x Wg[:d] + bg | x Wi + bi] for all N*F rows
// before it (fvta_linear_fwd), and d_facts, dWg, dWc, dWi, dbg, dbi as contractions over all N*F rows after the reverse
// recurrence (fvta_linear_bwd over the gate gradients the recurrence leaves in the workspace).
// The recurrence itself: row n's chain never reads another row, so a workgroup owns SEQ_RT = 16 rows (the M of
// v_mfma_f32_16x16x4_f32, exact fp32) and no workgroup ever waits for another.  Two regimes, by d:
//   A (dp = d rounded up to 16 <= 128): ONE launch for all F steps.  [Wg[d:] | Wc] stay in LDS for the whole launch,
//     as [unit][k] images with a row pad of 2 floats (conflict-free MFMA operand reads); the state tile stays on chip
//     (registers in the MFMA C layout + an LDS image as the next step's A operand).  A wave owns 16 units: r and hc of a
//     unit land in the same lane.  The backward keeps the same two matrices untransposed ([c][u] IS its [n][k] image).
//   B (larger d): the weights do not fit a CU, so a step is one fused launch over (row tiles x 64-unit column tiles): the
//     state-side product with the gate math as its epilogue; in the backward the gate gradient (recomputed per column
//     tile while the A operand is staged) with the d_h product.  Issued F times from one C call, ordered by the stream.
// No atomics, fixed summation order: two runs are bitwise equal.  The backward only reads `saved`.
#include "seq_common.h"

namespace fvta {

struct SeqFwdArgs {
  int N, F, d, dp;
  const float *gate, *h0, *Wg, *Wc, *preR, *preI;
  float *h_last, *S_h, *S_r, *S_hc, *S_hh;
};
struct SeqBwdArgs {
  int N, F, d, dp;
  const float *gate, *Wg, *Wc, *S_h, *S_r, *S_hc, *S_hh, *d_h_last;
  float *G_r, *G_c, *G_x, *d_gate, *d_h0;
};

// one element of the cell: returns h_t; r and hh come back for `saved` (the two fmafs: see "Rounding" in seq_common.h).
// A gate of 0 returns h itself.
__device__ __forceinline__ float seq_gate_fwd(float pre_r, float hc, float pre_i, float g, float h, float& r, float& hh) {
  r = fvta_sigmoid(pre_r);
  hh = fvta_tanh(fmaf(r, hc, pre_i));
  return fmaf(g, hh, (1.f - g) * h);
}
// gate gradient of one element: dr_pre, dhc, dxi; returns this element's share of d_gate
__device__ __forceinline__ float seq_gate_bwd(float dn, float g, float r, float hc, float hh, float h, float& dr, float& dhc,
                                              float& dxi) {
  const float dpre = dn * g * (1.f - hh * hh);
  dr = dpre * hc * r * (1.f - r);
  dhc = dpre * r;
  dxi = dpre;
  return dn * (hh - h);
}

// ---------------------------------------------------------------- regime A
// [Wg[d:] | Wc] into LDS for the whole launch, rows padded to dp and zero off the matrices: image[row][col] = W[row][col], or
// its transpose (TRANSPOSED: the forward's [u][k] = W[k][u]); either way consecutive threads read along a row of W
template <bool TRANSPOSED>
__device__ __forceinline__ void attgru_load_w(float* Wg_l, float* Wc_l, int ld, const float* Wg, const float* Wc, int d, int dp,
                                              int tid) {
  for (int idx = tid; idx < dp * dp; idx += 64 * SEQ_A_WAVES) {
    const int row = idx / dp, col = idx - row * dp, dst = TRANSPOSED ? col * ld + row : row * ld + col;
    const bool ok = row < d && col < d;
    const size_t src = ok ? (size_t)row * d + col : 0;
    const float vg = Wg[(size_t)d * d + src], vc = Wc[src];
    Wg_l[dst] = ok ? vg : 0.f;
    Wc_l[dst] = ok ? vc : 0.f;
  }
}

// grid ceil(N/16), 512 threads (a wave per 16-unit column tile), dynamic LDS (2 dp + 16) (dp + 2) floats
template <bool TRAIN>
__global__ __launch_bounds__(64 * SEQ_A_WAVES) void attgru_seq_fwd_a(SeqFwdArgs a) {
  extern __shared__ float smem[];
  const int N = a.N, F = a.F, d = a.d, dp = a.dp, ld = dp + 2;
  float* Wg_l = smem;             // [u][k] = Wg[d + k][u]
  float* Wc_l = Wg_l + dp * ld;   // [u][k] = Wc[k][u]
  float* H_l = Wc_l + dp * ld;    // [16][ld]: h_{t-1} of the tile
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int m0 = blockIdx.x * SEQ_RT;
  attgru_load_w<true>(Wg_l, Wc_l, ld, a.Wg, a.Wc, d, dp, tid);
  for (int idx = tid; idx < SEQ_RT * dp; idx += 64 * SEQ_A_WAVES) {
    const int i = idx / dp, u = idx - i * dp, n = m0 + i;
    float v = 0.f;
    if (a.h0 && n < N && u < d) v = a.h0[(size_t)n * d + u];
    H_l[i * ld + u] = v;
  }
  __syncthreads();
  const bool active = wave * 16 < dp;
  const auto [u, i0] = seq_lane(wave, lane);
  float h[4];
  bool ok[4];
  int64_t row[4];
  seq_lane_rows(m0, i0, u, N, d, ok, row);
#pragma unroll
  for (int r = 0; r < 4; ++r) h[r] = active ? H_l[(i0 + r) * ld + u] : 0.f;
  for (int t = 0; t < F; ++t) {
    float pr[4], pi[4], g[4];
    int64_t sidx[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {   // (state independent: issued ahead of the product)
      sidx[r] = ok[r] ? (row[r] * F + t) * d + u : 0;
      pr[r] = a.preR[sidx[r]];
      pi[r] = a.preI[sidx[r]];
      g[r] = a.gate[row[r] * F + t];
    }
    f32x4 acc_r = zero4(), acc_c = zero4();
    if (active) seq_mma2(H_l, ld, Wg_l + wave * 16 * ld, Wc_l + wave * 16 * ld, ld, dp, lane, acc_r, acc_c);
    __syncthreads();                // every wave has read H_l
    if (active) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float rr, hh;
        const float hn = seq_gate_fwd(acc_r[r] + pr[r], acc_c[r], pi[r], g[r], h[r], rr, hh);
        if (TRAIN && ok[r]) {
          a.S_h[sidx[r]] = h[r];
          a.S_r[sidx[r]] = rr;
          a.S_hc[sidx[r]] = acc_c[r];
          a.S_hh[sidx[r]] = hh;
        }
        h[r] = ok[r] ? hn : 0.f;
        H_l[(i0 + r) * ld + u] = h[r];
      }
    }
    __syncthreads();
  }
  seq_store_rows(a.h_last, h, ok, row, d, u);
}

// grid ceil(N/16), 512 threads, dynamic LDS (2 dp + 32) (dp + 2) + 128 floats
__global__ __launch_bounds__(64 * SEQ_A_WAVES) void attgru_seq_bwd_a(SeqBwdArgs a) {
  extern __shared__ float smem[];
  const int N = a.N, F = a.F, d = a.d, dp = a.dp, ld = dp + 2;
  float* Wg_l = smem;             // [c][u] = Wg[d + c][u]
  float* Wc_l = Wg_l + dp * ld;   // [c][u] = Wc[c][u]
  float* Tr = Wc_l + dp * ld;     // [16][ld]: dr of the step
  float* Tc = Tr + SEQ_RT * ld;   // [16][ld]: dhc
  float* part = Tc + SEQ_RT * ld; // [waves][16]: d_gate shares
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int m0 = blockIdx.x * SEQ_RT;
  attgru_load_w<false>(Wg_l, Wc_l, ld, a.Wg, a.Wc, d, dp, tid);
  const bool active = wave * 16 < dp;
  const auto [u, i0] = seq_lane(wave, lane);
  float dn[4];
  bool ok[4];
  int64_t row[4];
  seq_lane_rows(m0, i0, u, N, d, ok, row);
#pragma unroll
  for (int r = 0; r < 4; ++r) dn[r] = ok[r] ? a.d_h_last[row[r] * d + u] : 0.f;
  __syncthreads();
  for (int t = F - 1; t >= 0; --t) {
    f32x4 acc0, acc1 = zero4();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t sidx = ok[r] ? (row[r] * F + t) * d + u : 0;
      const float g = a.gate[row[r] * F + t];
      const float rr = a.S_r[sidx], hc = a.S_hc[sidx], hh = a.S_hh[sidx], hp = a.S_h[sidx];
      float dr, dhc, dxi;
      float pg = seq_gate_bwd(dn[r], g, rr, hc, hh, hp, dr, dhc, dxi);   // (dn is 0 off the tensor: all of these are 0 there)
      if (ok[r]) {
        a.G_r[sidx] = dr;
        a.G_c[sidx] = dhc;
        a.G_x[sidx] = dxi;
      }
      if (active) {
        Tr[(i0 + r) * ld + u] = dr;
        Tc[(i0 + r) * ld + u] = dhc;
      }
      pg = row16_sum(pg);           // over the wave's 16 units of row i0 + r
      if ((lane & 15) == 0) part[wave * SEQ_RT + i0 + r] = pg;
      acc0[r] = dn[r] * (1.f - g);
    }
    __syncthreads();
    if (active) seq_mma_ab(Tr, Tc, ld, Wg_l + wave * 16 * ld, Wc_l + wave * 16 * ld, ld, dp, lane, acc0, acc1);
    if (tid < SEQ_RT && m0 + tid < N) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < SEQ_A_WAVES; ++w) s += part[w * SEQ_RT + tid];
      a.d_gate[(int64_t)(m0 + tid) * F + t] = s;
    }
    __syncthreads();                // Tr / Tc / part are free again
#pragma unroll
    for (int r = 0; r < 4; ++r) dn[r] = ok[r] ? acc0[r] + acc1[r] : 0.f;
  }
  seq_store_rows(a.d_h0, dn, ok, row, d, u);
}

// ---------------------------------------------------------------- regime B
// One step.  grid (ceil(N/16), ceil(d/64)), 256 threads.  h_prev [N] rows of stride ldp (NULL: zeros), h_new of stride ldn.
template <bool TRAIN>
__global__ __launch_bounds__(256) void attgru_seq_fwd_b(SeqFwdArgs a, int t, const float* __restrict__ h_prev, int64_t ldp,
                                                        float* __restrict__ h_new, int64_t ldn, int store_prev) {
  __shared__ float A_l[SEQ_RT * SEQ_B_LD], Bg_l[SEQ_B_CT * SEQ_B_LD], Bc_l[SEQ_B_CT * SEQ_B_LD];
  const int N = a.N, F = a.F, d = a.d;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int m0 = blockIdx.x * SEQ_RT, c0 = blockIdx.y * SEQ_B_CT;
  f32x4 acc_r = zero4(), acc_c = zero4();
  for (int k0 = 0; k0 < d; k0 += SEQ_B_KC) {
    seq_stage_a(A_l, h_prev, ldp, N, d, m0, k0, tid);
    seq_stage_w2<false>(Bg_l, Bc_l, a.Wg + (size_t)d * d, a.Wc, d, d, c0, k0, tid);
    __syncthreads();
    seq_mma2(A_l, SEQ_B_LD, Bg_l + wave * 16 * SEQ_B_LD, Bc_l + wave * 16 * SEQ_B_LD, SEQ_B_LD, SEQ_B_KC, lane, acc_r, acc_c);
    __syncthreads();
  }
  const auto [u, i0] = seq_lane(wave, lane, c0);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = m0 + i0 + r;
    if (seq_live(n, u, N, d)) {
      const int64_t sidx = ((int64_t)n * F + t) * d + u;
      const float hp = h_prev ? h_prev[(int64_t)n * ldp + u] : 0.f;
      float rr, hh;
      const float hn = seq_gate_fwd(acc_r[r] + a.preR[sidx], acc_c[r], a.preI[sidx], a.gate[(int64_t)n * F + t], hp, rr, hh);
      if (TRAIN) {
        if (store_prev) a.S_h[sidx] = hp;
        a.S_r[sidx] = rr;
        a.S_hc[sidx] = acc_c[r];
        a.S_hh[sidx] = hh;
      }
      h_new[(int64_t)n * ldn + u] = hn;
    }
  }
}

// One reverse step.  grid as above.  d_cur / d_next [N,d] (d_next differs from d_cur: other column tiles read d_cur)
__global__ __launch_bounds__(256) void attgru_seq_bwd_b(SeqBwdArgs a, int t, const float* __restrict__ d_cur,
                                                        float* __restrict__ d_next) {
  __shared__ float Tr[SEQ_RT * SEQ_B_LD], Tc[SEQ_RT * SEQ_B_LD], Bg_l[SEQ_B_CT * SEQ_B_LD], Bc_l[SEQ_B_CT * SEQ_B_LD];
  const int N = a.N, F = a.F, d = a.d;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int m0 = blockIdx.x * SEQ_RT, c0 = blockIdx.y * SEQ_B_CT;
  const bool first = blockIdx.y == 0;   // the column tile that also writes the gate gradients and d_gate
  f32x4 acc0 = zero4(), acc1 = zero4();
  float pg[2] = {0.f, 0.f};
  for (int k0 = 0; k0 < d; k0 += SEQ_B_KC) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      int i, kk;
      seq_b_decode(tid, p, i, kk);
      const int n = m0 + i, uu = k0 + kk;
      float dr = 0.f, dhc = 0.f, dxi = 0.f;
      if (n < N && uu < d) {
        const int64_t sidx = ((int64_t)n * F + t) * d + uu;
        pg[p] += seq_gate_bwd(d_cur[(int64_t)n * d + uu], a.gate[(int64_t)n * F + t], a.S_r[sidx], a.S_hc[sidx], a.S_hh[sidx],
                              a.S_h[sidx], dr, dhc, dxi);
        if (first) {
          a.G_r[sidx] = dr;
          a.G_c[sidx] = dhc;
          a.G_x[sidx] = dxi;
        }
      }
      Tr[i * SEQ_B_LD + kk] = dr;
      Tc[i * SEQ_B_LD + kk] = dhc;
    }
    seq_stage_w2<true>(Bg_l, Bc_l, a.Wg + (size_t)d * d, a.Wc, d, d, c0, k0, tid);
    __syncthreads();
    seq_mma_ab(Tr, Tc, SEQ_B_LD, Bg_l + wave * 16 * SEQ_B_LD, Bc_l + wave * 16 * SEQ_B_LD, SEQ_B_LD, SEQ_B_KC, lane, acc0, acc1);
    __syncthreads();
  }
#pragma unroll
  for (int p = 0; p < 2; ++p) {     // row i = (tid >> 5) + 8 p lives in one 32-lane half: fixed-order tree inside it
    float s = pg[p];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);   // (row16_sum adds in another order: other bits)
    const int n = m0 + (tid >> 5) + 8 * p;
    if (first && (tid & 31) == 0 && n < N) a.d_gate[(int64_t)n * F + t] = s;
  }
  const auto [u, i0] = seq_lane(wave, lane, c0);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = m0 + i0 + r;
    if (seq_live(n, u, N, d))
      d_next[(int64_t)n * d + u] = d_cur[(int64_t)n * d + u] * (1.f - a.gate[(int64_t)n * F + t]) + acc0[r] + acc1[r];
  }
}

// seq_common.h's fill, for gru_seq.hip too.  grid 64, 256 threads
__global__ __launch_bounds__(256) void seq_zero_params_kernel(SeqZeroTable t) {
#pragma unroll
  for (int j = 0; j < 5; ++j)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < t.n[j]; i += (int64_t)gridDim.x * 256) t.p[j][i] = 0.f;
}
void seq_zero_params(const SeqZeroTable& t, hipStream_t s) { hipLaunchKernelGGL(seq_zero_params_kernel, dim3(64), dim3(256), 0, s, t); }

static inline size_t seq_lds_fwd_a(int dp) { return (size_t)(2 * dp + SEQ_RT) * (dp + 2) * sizeof(float); }
static inline size_t seq_lds_bwd_a(int dp) {
  return ((size_t)(2 * dp + 2 * SEQ_RT) * (dp + 2) + SEQ_A_WAVES * SEQ_RT) * sizeof(float);
}
static_assert((2 * SEQ_A_DP_MAX + 2 * SEQ_RT) * (SEQ_A_DP_MAX + 2) * 4 + SEQ_A_WAVES * SEQ_RT * 4 <= 160 * 1024,
              "regime A's weights and tiles must fit the 160 KiB of a CU");

static inline size_t attgru_n(const fvta_attgru_seq_desc& d) { return (size_t)d.N * d.F * d.d; }
// saved: h_{t-1}, r, hc, hh.  workspace, forward: pre_r (a), pre_i (b), two state rows (regime B without `saved`); backward:
// the gate gradients dr (a), dhc (b), dxi (c), two d_h rows
static inline SeqWork attgru_work(const fvta_attgru_seq_desc& d, int backward, void* p) {
  return SeqWork(attgru_n(d), (size_t)d.N * d.d, 1, backward != 0, p);
}

static inline bool seq_desc_ok(const fvta_attgru_seq_desc* d) { return d && d->N > 0 && d->F > 0 && d->d > 0; }

}  // namespace fvta
using namespace fvta;

extern "C" size_t fvta_attgru_seq_saved_bytes(const fvta_attgru_seq_desc* d) {
  if (!seq_desc_ok(d)) return seq_refuse("attgru_seq_saved_bytes: bad N/F/d");
  return d->training ? SeqSaved(attgru_n(*d), nullptr).bytes : 0;
}

extern "C" size_t fvta_attgru_seq_workspace_bytes(const fvta_attgru_seq_desc* d, int32_t backward) {
  if (!seq_desc_ok(d)) return seq_refuse("attgru_seq_workspace_bytes: bad N/F/d");
  return attgru_work(*d, backward, nullptr).bytes;
}

extern "C" int fvta_attgru_seq_plan(const fvta_attgru_seq_desc* d, int32_t* out) {
  FVTA_CHECK_ARG(seq_desc_ok(d), "attgru_seq_plan: bad N/F/d");
  FVTA_CHECK_ARG(out, "attgru_seq_plan: null pointer");
  seq_fill_plan(out, seq_regime_a(d->d), 1, d->F);
  return FVTA_OK;
}

extern "C" int fvta_attgru_seq_fwd(const fvta_attgru_seq_desc* d, const float* facts, const float* gate, const float* h0,
                                   const float* Wg, const float* bg, const float* Wc, const float* Wi, const float* bi,
                                   float* h_last, void* saved, void* workspace, fvta_stream_t stream_) {
  FVTA_CHECK_ARG(seq_desc_ok(d), "attgru_seq_fwd: bad N/F/d");
  FVTA_CHECK_ARG(facts && gate && Wg && bg && Wc && Wi && bi && h_last && workspace, "attgru_seq_fwd: null pointer");
  FVTA_CHECK_ARG(!d->training || saved, "attgru_seq_fwd: training wants `saved`");
  hipStream_t s = (hipStream_t)stream_;
  const int N = d->N, F = d->F, dd = d->d;
  const SeqWork w = attgru_work(*d, 0, workspace);
  const SeqSaved sv(attgru_n(*d), d->training ? saved : nullptr);
  const int64_t M = (int64_t)N * F;
  int st = fvta_linear_fwd(facts, Wg, bg, w.a, M, dd, dd, 0, stream_);   // x Wg[:d] + bg  (attention_gru_cell.py:63)
  if (st != FVTA_OK) return st;
  st = fvta_linear_fwd(facts, Wi, bi, w.b, M, dd, dd, 0, stream_);       // x Wi + bi      (:68)
  if (st != FVTA_OK) return st;
  SeqFwdArgs a{N, F, dd, seq_dp(dd), gate, h0, Wg, Wc, w.a, w.b, h_last, sv.s[0], sv.s[1], sv.s[2], sv.s[3]};
  const unsigned row_tiles = seq_row_tiles(N);
  if (seq_regime_a(dd)) {
    const size_t lds = seq_lds_fwd_a(a.dp);
    if (d->training) {
      fvta_allow_lds(attgru_seq_fwd_a<true>, lds);
      hipLaunchKernelGGL(attgru_seq_fwd_a<true>, dim3(row_tiles), dim3(64 * SEQ_A_WAVES), lds, s, a);
    } else {
      fvta_allow_lds(attgru_seq_fwd_a<false>, lds);
      hipLaunchKernelGGL(attgru_seq_fwd_a<false>, dim3(row_tiles), dim3(64 * SEQ_A_WAVES), lds, s, a);
    }
  } else {
    const dim3 grid = seq_grid_b(N, dd);
    const int64_t lds_saved = (int64_t)F * dd;
    float* buf[2] = {w.s0, w.s1};
    for (int t = 0; t < F; ++t) {
      const bool last = t + 1 == F;
      if (d->training) {   // h_t goes straight into the next step's slot of `saved`
        const float* hp = t == 0 ? h0 : sv.s[0] + (size_t)t * dd;
        float* hn = last ? h_last : sv.s[0] + (size_t)(t + 1) * dd;
        hipLaunchKernelGGL(attgru_seq_fwd_b<true>, grid, dim3(256), 0, s, a, t, hp, t == 0 ? (int64_t)dd : lds_saved, hn,
                           last ? (int64_t)dd : lds_saved, t == 0 ? 1 : 0);
      } else {
        const float* hp = t == 0 ? h0 : buf[t & 1];
        float* hn = last ? h_last : buf[(t + 1) & 1];
        hipLaunchKernelGGL(attgru_seq_fwd_b<false>, grid, dim3(256), 0, s, a, t, hp, (int64_t)dd, hn, (int64_t)dd, 0);
      }
    }
  }
  FVTA_CHECK_LAUNCH("attgru_seq_fwd");
  return FVTA_OK;
}

extern "C" int fvta_attgru_seq_bwd(const fvta_attgru_seq_desc* d, const float* facts, const float* gate, const float* Wg,
                                   const float* Wc, const float* Wi, const void* saved, const float* d_h_last,
                                   float* d_facts, float* d_gate, float* d_h0, float* dWg, float* dbg, float* dWc,
                                   float* dWi, float* dbi, int32_t accumulate, void* workspace, fvta_stream_t stream_) {
  FVTA_CHECK_ARG(seq_desc_ok(d), "attgru_seq_bwd: bad N/F/d");
  FVTA_CHECK_ARG(d->training, "attgru_seq_bwd: the forward ran with training = 0, nothing was saved");
  FVTA_CHECK_ARG(facts && gate && Wg && Wc && Wi && saved && d_h_last && d_facts && d_gate && dWg && dbg && dWc && dWi &&
                     dbi && workspace,
                 "attgru_seq_bwd: null pointer");
  hipStream_t s = (hipStream_t)stream_;
  const int N = d->N, F = d->F, dd = d->d;
  const SeqWork w = attgru_work(*d, 1, workspace);
  const SeqSaved sv(attgru_n(*d), const_cast<void*>(saved));
  const int64_t dsq = (int64_t)dd * dd;
  if (!accumulate) seq_zero_params({{dWg, dWc, dWi, dbg, dbi}, {2 * dsq, dsq, dsq, dd, dd}}, s);
  SeqBwdArgs a{N, F, dd, seq_dp(dd), gate, Wg, Wc, sv.s[0], sv.s[1], sv.s[2], sv.s[3], d_h_last, w.a, w.b, w.c, d_gate, d_h0};
  const unsigned row_tiles = seq_row_tiles(N);
  if (seq_regime_a(dd)) {
    const size_t lds = seq_lds_bwd_a(a.dp);
    fvta_allow_lds(attgru_seq_bwd_a, lds);
    hipLaunchKernelGGL(attgru_seq_bwd_a, dim3(row_tiles), dim3(64 * SEQ_A_WAVES), lds, s, a);
  } else {
    const dim3 grid = seq_grid_b(N, dd);
    float* buf[2] = {w.s0, w.s1};
    const float* cur = d_h_last;
    for (int t = F - 1; t >= 0; --t) {
      float* nxt = (t == 0 && d_h0) ? d_h0 : buf[t & 1];
      hipLaunchKernelGGL(attgru_seq_bwd_b, grid, dim3(256), 0, s, a, t, cur, nxt);
      cur = nxt;
    }
  }
  FVTA_CHECK_LAUNCH("attgru_seq_bwd");
  // contractions over all N*F rows: d_facts = dr Wg[:d]^T + dxi Wi^T; dWg[:d], dbg, dWi, dbi from x; dWg[d:], dWc from h_{t-1}
  const int64_t M = (int64_t)N * F;
  int st = fvta_linear_bwd(facts, Wg, nullptr, w.a, d_facts, dWg, dbg, M, dd, dd, 0, 0, stream_);
  if (st != FVTA_OK) return st;
  st = fvta_linear_bwd(facts, Wi, nullptr, w.c, d_facts, dWi, dbi, M, dd, dd, 0, 1, stream_);
  if (st != FVTA_OK) return st;
  st = fvta_linear_bwd(sv.s[0], Wg + dsq, nullptr, w.a, nullptr, dWg + dsq, nullptr, M, dd, dd, 0, 0, stream_);
  if (st != FVTA_OK) return st;
  return fvta_linear_bwd(sv.s[0], Wc, nullptr, w.b, nullptr, dWc, nullptr, M, dd, dd, 0, 0, stream_);
}
