// Focal attention backward for MANY QUESTIONS OVER ONE ALBUM (fvta_attn_shared_bwd): the gradient of
// fvta_attn_shared_fwd_train.  For question i: d_hq[i] and i's share of dW / db are fvta_attn_bwd's (accumulate = 0) on the
// pair (hinfo[album[i]], hq[i]); d_hinfo[a] is the sum of those calls' row gradients over the questions of album a -- with
// no [NQ,K,T,w] tensor anywhere: the rows stay [A,K,T,w] on both sides.  simiMatrix 1-3.
//
// As in attn_bwd.hip the max over j leaves ONE (t, j) pair per row and question with gradient:
//   dh[t]      = sum_q  p_q[t] r_q[k] g_q  +  dx_q[t] (Qs_q[jmax_q[t]] + Rh + 2 R2 h[t])
//   dQs_q[j]  += dx_q[t] h[t]   for j = jmax_q[t];   d ct_q[j] += dx_q[t];   d Rh += (sum_q dx_q[t]) h[t], d R2 likewise h^2
// Launches, all on the caller's stream, none waits for the host, no memset:
//   1. attn_shared_bwd_prep_kernel    per question: gu[k] = g.u[k], the tie count of amax == M, coef = r / L, ds[k] / ties
//   2. attn_shared_bwd_rows_kernel    one workgroup per (album, k, chunk of row tiles): a tile's rows in registers, the
//                                     album's questions in plan order (ascending question index: the training plan);
//                                     per question g_q.h[t], p, dx -> dx [NQ,K,T]; dh accumulated in registers and every
//                                     d_hinfo row stored ONCE (zeros for an album without a question and for masked rows
//                                     that no fully masked question weights); d Rh / d R2 partials per workgroup.
//                                     The Qs gather (one 16-byte piece per thread, row and question) is served from L2
//   3. attn_shared_bwd_q_kernel       one wave per (group, slice of 32 channels, split of T): the group's G JP = 256
//                                     accumulator rows x 32 channels in LDS (32 KB), a lane owns (question, 4 channels)
//                                     and with them a private column of LDS: no barrier in the sweep.  Rows in (k, t)
//                                     order: acc[(g, jmax_g[t])] += dx_g[t] h[t]; d ct likewise.  Partials per split.
//                                     A group of fewer than G questions spreads each question's rows over the free
//                                     regions (runs of four rows, round robin) and adds the regions in order
//   4. attn_shared_bwd_fold_kernel    per (question, 8 positions, 256 channels): the splits in order; d_hq = U dQs +
//                                     dct (Cq + 2 C2 q); parameter-vector partials per (question, 8 positions)
//   5. attn_shared_bwd_params_kernel  all partials in index order -> dW / db through attn_common.h's mapping
// Row traffic: (2) reads each row once and writes its gradient once; (3) reads each row once per group of its album.
// Determinism: no floating-point atomics.  The chunks, slices and splits depend on the descriptor only
// (fvta_attn_shared_bwd_plan); the one sum whose order depends on data -- d_hinfo over an album's questions -- runs in
// `order`, which the training plan fills by ascending question index (attn_shared.hip: attn_shared_plan_kernel<true>).
// Kernels 1, 4 and 5 are a few lines each around attn_bwd_shared.h's prep body, fold body and parameter pieces -- the one
// copy attn_bwd.hip runs too; the row and question passes (2, 3), the backward's shape and its workspace stand in
// attn_shared_bwd_kernels.h, with the compile-time word POOL for training over per-question album lists (attn_pool.hip).
// ONE driver makes the launches for the four backward entry points: shb_backward, near the end of this file.
// Under the time warp (fvta_attn_shared_bwd_tw, the gradient of fvta_attn_shared_fwd_tw_train): the TW instantiations of
// (2) and (3) and six small kernels of the warp's own backward, at the end of this file.  Over the pool under the warp
// (fvta_attn_pool_bwd_tw): <TW, POOL> of (2) and (3), and of the warp's kernels (b) and (c) their POOL instantiations.
#include "attn_shared_bwd_kernels.h"
#include "timewarp_common.h"

namespace fvta {

constexpr int SHB_E_WGS = 512;        // at most this many workgroups of the energy backward: one dv partial each

// ---- per-(question, k) scalars: attn_bwd_shared.h's prep body on the shared forward's `saved`.  grid NQ; a wave per k
__global__ __launch_bounds__(1024) void attn_shared_bwd_prep_kernel(ShShape s, ShWork sv, ShBwdWork wk,
                                                                   const float* __restrict__ d_h_a) {
  const size_t q = blockIdx.x, qk = q * s.K;
  // a (question, k) without a valid (t, j) pair has M = -1e30: nothing passes into its masked logits
  const bool allmasked = (int)threadIdx.x < s.K && sv.M[qk + threadIdx.x] == FVTA_NEG;
  attn_bwd_prep_body(d_h_a + q * s.w, sv.u + qk * s.w, sv.M + qk, sv.amax + qk * s.T, sv.r + qk, sv.L + qk, allmasked, s.w, s.K,
                     s.T, wk.coef + qk, wk.gu + qk, wk.dss + qk);
}

// ---- fold (attn_bwd_shared.h: attn_bwd_fold_body).  grid (NQ, ceil(w / 256), JZ); the question's TS splits in order
__global__ __launch_bounds__(256) void attn_shared_bwd_fold_kernel(ShShape s, ShBwdShape bs, ShWork sv, ShBwdWork wk,
                                                                  const float* __restrict__ hq, float* __restrict__ d_hq) {
  const int q = blockIdx.x, c = blockIdx.y * 256 + 4 * (threadIdx.x & 63);
  const int w = s.w, JP = s.JP, JQ = s.JQ, TS = bs.TS;
  int slot = sv.qslot[q];
  slot = min(max(slot, 0), s.ngmax * s.G - 1);
  const int grp = slot / s.G, g = slot % s.G;
  const size_t row0 = (size_t)grp * TS * SH_BN + (size_t)g * JP;  // + ts * SH_BN + j
  const bool live = c < w;
  f32x4 pU, pCq, pC2;
  if (!attn_bwd_fold_body(sv.vecs, hq + (size_t)q * JQ * w, d_hq + (size_t)q * JQ * w, false, wk.dctp + row0, (size_t)SH_BN, TS,
                          wk.dctn + (size_t)q * JP, w, JP, JQ,
                          [&](int j) {
                            return attn_bwd_slot_sum<f32x4>(
                                TS, [&](int ts) { return ld4_if(live, wk.qpart + (row0 + (size_t)ts * SH_BN + j) * w + c); });
                          },
                          pU, pCq, pC2))
    return;
  float* pv = wk.pvec + ((size_t)q * bs.JZ + blockIdx.z) * 3 * w;  // (no d Rh / d R2 here: the row pass leaves them per slot)
  *reinterpret_cast<f32x4*>(pv + c) = pU;
  *reinterpret_cast<f32x4*>(pv + w + c) = pCq;
  *reinterpret_cast<f32x4*>(pv + 2 * w + c) = pC2;
}

// ---- parameters (attn_bwd_shared.h: the parameter kernels' pieces).  grid ceil(w / 64) + 1; all partials in index order
__global__ __launch_bounds__(256) void attn_shared_bwd_params_kernel(ShShape s, ShBwdShape bs, ShBwdWork wk,
                                                                    float* __restrict__ dW, float* __restrict__ db) {
  if (blockIdx.x == gridDim.x - 1) {
    attn_bwd_bias_block(wk.dctn, (size_t)s.NQ * s.JP, db);
    return;
  }
  const int part = threadIdx.x >> 6, w = s.w, c = blockIdx.x * 64 + (threadIdx.x & 63);
  float v[VEC_COUNT] = {0, 0, 0, 0, 0};
  if (c < w) {
    const size_t qrows = (size_t)s.NQ * bs.JZ, slots = (size_t)s.A * s.K * bs.nch * bs.RH;
    v[VEC_U] = attn_bwd_sum_rows(wk.pvec, qrows, 3, 0, part, w, c);
    v[VEC_CQ] = attn_bwd_sum_rows(wk.pvec, qrows, 3, 1, part, w, c);
    v[VEC_C2] = attn_bwd_sum_rows(wk.pvec, qrows, 3, 2, part, w, c);
    v[VEC_RH] = attn_bwd_sum_rows(wk.rowp, slots, 2, 0, part, w, c);
    v[VEC_R2] = attn_bwd_sum_rows(wk.rowp, slots, 2, 1, part, w, c);
  }
  attn_bwd_combine_dW(v, s.simi, 0, w, c, dW);
}

// ================= under the time warp (fvta_attn_shared_bwd_tw): the gradient of fvta_attn_shared_fwd_tw_train ==========
// The attention saw the rows s h, s[q,t] = tanh(z[q,t]) cnt(t), z = e[a,t] + K (s0 + WC.lq[q]).  The row and question passes
// above run as their TW instantiations and leave ds [NQ,K,T]; from there the warp's own backward, which never meets a
// [NQ,K,T,w] tensor either: s is one scalar per (question, position) and only e reads the rows.
// POOL: z[q, m T + j] = e[albums[q,m], j] + K (s0 + WC.lq[q]) over the question's TO = M T positions, the count that of the
// global position; (b) runs over TO, (c) sums an album's references, (d) - (f) are what they are with A = P, T = JX.
//   a. attn_shared_tw_vec_kernel        v = WH[:w] WC (attn_shared.hip's)
//   b. attn_shared_bwd_tw_dz_kernel     per question: dz[q,t] = cnt(t) (1 - tanh(z)^2) sum_k ds[q,k,t] (k in index order),
//                                       Dq[q] = K sum_t dz[q,t] by a fixed tree, d_lq[q] = Dq[q] WC; dbq[q] = sum dbt
//   c. attn_shared_bwd_tw_de_kernel     de[a,t] = sum of dz[q,t] over the album's questions in plan order (ascending q)
//   d. attn_shared_bwd_tw_energy_kernel a wave per (album, t), all K rows: d_hinfo += 2 de v h (masked rows too: e sums
//                                       them), dv partials per workgroup.  An album without a question is skipped: its de
//                                       is 0 and the row pass has stored its zeros.  One more read of the rows and one
//                                       read-modify-write of d_hinfo: de depends on every k and every question of the album
//   e. attn_shared_bwd_tw_dv_kernel     dv = the partials in index order; ds0 = sum_q Dq[q]; db += sum_q dbq[q]
//   f. attn_shared_bwd_tw_params_kernel dWH_W[:w] += dv (x) WC, dWH_b += ds0 WC, dWC_W += WH^T dv + ds0 b_WH + Dq^T lq,
//                                       dWC_b += ds0
// Over the pool (fvta_attn_pool_bwd_tw) these arrays stand past the pooled backward's dctq (PoolBwdWork), and what is per
// question runs over its TO = M T positions; de stays per pooled album.  Not pooled, TO = T: every address is what it was
struct ShBwdTwWork {
  ShBwdWork base;
  float *ds, *dxs, *dbt;  // [NQ,K,TO]
  float* dz;        // [NQ,TO]
  float* de;        // [A,T]
  float* Dq;        // [NQ]  K sum_t dz
  float* dbq;       // [NQ]  sum_{k,t} dbt
  float* v;         // [w]
  float* dvp;       // [ewg][w]
  float* dv;        // [w]
  float* ds0;       // [1]
  int ewg;
  size_t bytes;
  ShBwdTwWork(const ShShape& s, const ShBwdShape& b, void* p, bool pool = false) : base(s, b, p) {
    FvtaCarver c(p);
    c.off = pool ? PoolBwdWork(s, b, p).bytes : base.bytes;
    const size_t nk = (size_t)s.NQ * s.K;
    const int64_t waves = ((int64_t)s.A * s.T + 3) / 4;
    ewg = (int)(waves < SHB_E_WGS ? waves : SHB_E_WGS);
    ds = c.take<float>(nk * s.TO);
    dxs = c.take<float>(nk * s.TO);
    dbt = c.take<float>(nk * s.TO);
    dz = c.take<float>((size_t)s.NQ * s.TO);
    de = c.take<float>((size_t)s.A * s.T);
    Dq = c.take<float>((size_t)s.NQ);
    dbq = c.take<float>((size_t)s.NQ);
    v = c.take<float>((size_t)s.w);
    dvp = c.take<float>((size_t)ewg * s.w);
    dv = c.take<float>((size_t)s.w);
    ds0 = c.take<float>(1);
    bytes = c.off;
  }
};

// the workgroup's 256 values, added by a fixed tree; the result in every thread (the leading barrier: a second call may
// not write while a thread still reads the first one's result)
__device__ __forceinline__ float shb_block_tree_sum(float v) {
  __shared__ float s_red[256];
  __syncthreads();
  s_red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s_red[threadIdx.x] += s_red[threadIdx.x + o];
    __syncthreads();
  }
  return s_red[0];
}

// ---- b.  grid NQ, 256 threads
// POOL: over the question's TO = M T positions, the count that of the GLOBAL position t = m T + j, as the forward's scale
// kernel takes it.  No row pass visits the positions of an empty slot (qslot < 0: the plan's word for albums[q,m] < 0), so
// their ds / dbt hold whatever the workspace held: they are not read.  dz = 0 there is the true value -- an empty slot is
// T zero rows and ds a dot product with them -- and dbt's share is 0 for the same reason
template <bool POOL>
__global__ __launch_bounds__(256) void attn_shared_bwd_tw_dz_kernel(ShShape s, const int* __restrict__ qslot, int warp_type, int win,
                                                                   const float* __restrict__ tz, const float* __restrict__ WC,
                                                                   ShBwdTwWork wk, float* __restrict__ d_lq) {
  const int q = blockIdx.x, tid = threadIdx.x, T = sh_positions<POOL>(s), K = s.K;
  float acc = 0.f, accb = 0.f;
  for (int t = tid; t < T; t += 256) {
    if constexpr (POOL)
      if (qslot[(size_t)q * s.M + t / s.T] < 0) {
        wk.dz[(size_t)q * T + t] = 0.f;
        continue;
      }
    float sum = 0.f;
    for (int k = 0; k < K; ++k) {
      sum += wk.ds[((size_t)q * K + k) * T + t];
      accb += wk.dbt[((size_t)q * K + k) * T + t];
    }
    const float c = tz[(size_t)q * T + t];
    const float dz = sum * tw_count(t, T, warp_type, win) * (1.f - c * c);
    wk.dz[(size_t)q * T + t] = dz;
    acc += dz;
  }
  const float D = shb_block_tree_sum(acc) * (float)K;
  const float dbq = shb_block_tree_sum(accb);
  if (tid == 0) {
    wk.Dq[q] = D;
    wk.dbq[q] = dbq;
  }
  for (int c = tid; c < s.w; c += 256) d_lq[(size_t)q * s.w + c] = D * WC[c];
}

// ---- c.  grid (A, ceil(T / 256)), 256 threads
// POOL: over the pooled album's references in plan order (ascending id q M + m), each read at its slot of its question's
// TO positions; a question that lists the album twice stands twice in the sum
template <bool POOL>
__global__ __launch_bounds__(256) void attn_shared_bwd_tw_de_kernel(ShShape s, ShWork sv, ShBwdTwWork wk) {
  const int a = blockIdx.x, t = blockIdx.y * 256 + threadIdx.x;
  if (t >= s.T) return;
  const int TP = sh_positions<POOL>(s), NRF = POOL ? s.NR : s.NQ;
  const int q0 = min(max(sv.astart[a], 0), NRF), nqa = min(sv.acnt[a], NRF - q0);
  float acc = 0.f;
  for (int qi = 0; qi < nqa; ++qi) {
    int ref = sv.order[q0 + qi];
    ref = ref < 0 ? 0 : (ref >= NRF ? NRF - 1 : ref);
    acc += wk.dz[(size_t)sh_ref_q<POOL>(s, ref) * TP + sh_ref_off<POOL>(s, ref) + t];
  }
  wk.de[(size_t)a * s.T + t] = acc;
}

// ---- d.  grid ewg, 256 threads: a wave per (album, t), positions strided over the waves; lane l holds channels
// 256 g + 4 l .. + 3 (CPT = max(1, w / 256) quads)
template <int CPT>
__global__ __launch_bounds__(256) void attn_shared_bwd_tw_energy_kernel(ShShape s, ShWork sv, ShBwdTwWork wk,
                                                                       const float* __restrict__ hinfo,
                                                                       float* __restrict__ d_hinfo) {
  __shared__ f32x4 s_dv[3][CPT][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t npos = (int64_t)s.A * s.T, nwv = (int64_t)gridDim.x * 4;
  const int w = s.w;
  f32x4 v[CPT], dvacc[CPT];
#pragma unroll
  for (int g = 0; g < CPT; ++g) {
    v[g] = 256 * g + 4 * lane < w ? ld4(wk.v + 256 * g + 4 * lane) : zero4();
    dvacc[g] = zero4();
  }
  for (int64_t pos = (int64_t)blockIdx.x * 4 + wave; pos < npos; pos += nwv) {
    const int a = (int)(pos / s.T), t = (int)(pos % s.T);
    if (sv.acnt[a] <= 0) continue;  // (wave-uniform; no barrier inside the loop)
    const float de = wk.de[pos];
    for (int k = 0; k < s.K; ++k) {
      const size_t ro = (((size_t)a * s.K + k) * s.T + t) * w + 4 * lane;
#pragma unroll
      for (int g = 0; g < CPT; ++g)
        if (256 * g + 4 * lane < w) {
          const f32x4 h = ld4(hinfo + ro + 256 * g);
          f32x4* dst = reinterpret_cast<f32x4*>(d_hinfo + ro + 256 * g);
          *dst = *dst + h * v[g] * (2.f * de);
          dvacc[g] += h * h * de;
        }
    }
  }
  if (wave)
#pragma unroll
    for (int g = 0; g < CPT; ++g) s_dv[wave - 1][g][lane] = dvacc[g];
  __syncthreads();
  if (wave) return;
#pragma unroll
  for (int g = 0; g < CPT; ++g)
    if (256 * g + 4 * lane < w) {
      f32x4 acc = dvacc[g];
#pragma unroll
      for (int u = 0; u < 3; ++u) acc += s_dv[u][g][lane];
      *reinterpret_cast<f32x4*>(wk.dvp + (size_t)blockIdx.x * w + 256 * g + 4 * lane) = acc;
    }
}

// ---- e.  grid ceil(w / 64) + 1, 256 threads = 64 channels x 4 thread groups; the last block: ds0 and db
__global__ __launch_bounds__(256) void attn_shared_bwd_tw_dv_kernel(ShShape s, ShBwdTwWork wk, float* __restrict__ db) {
  if (blockIdx.x == gridDim.x - 1) {
    float acc = 0.f, accb = 0.f;
    for (int q = threadIdx.x; q < s.NQ; q += 256) {
      acc += wk.Dq[q];
      accb += wk.dbq[q];
    }
    acc = shb_block_tree_sum(acc);
    accb = shb_block_tree_sum(accb);
    if (threadIdx.x == 0) {
      wk.ds0[0] = acc;
      db[0] += accb;
    }
    return;
  }
  __shared__ float s_p[4][64];
  const int part = threadIdx.x >> 6, cl = threadIdx.x & 63, c = blockIdx.x * 64 + cl;
  s_p[part][cl] = c < s.w ? attn_bwd_sum_rows(wk.dvp, (size_t)wk.ewg, 1, 0, part, s.w, c) : 0.f;
  __syncthreads();
  if (part == 0 && c < s.w) wk.dv[c] = (s_p[0][cl] + s_p[1][cl]) + (s_p[2][cl] + s_p[3][cl]);
}

// ---- f.  grid ceil(w / 64), 256 threads = 64 columns o x 4 thread groups over the rows (WH: [.,w] row-major, the first w rows)
__global__ __launch_bounds__(256) void attn_shared_bwd_tw_params_kernel(ShShape s, ShBwdTwWork wk, const float* __restrict__ WH,
                                                                       const float* __restrict__ WHb, const float* __restrict__ WC,
                                                                       const float* __restrict__ lq, float* __restrict__ dWH,
                                                                       float* __restrict__ dWHb, float* __restrict__ dWC,
                                                                       float* __restrict__ dWCb) {
  __shared__ float s_p[4][64];
  const int part = threadIdx.x >> 6, cl = threadIdx.x & 63, o = blockIdx.x * 64 + cl, w = s.w;
  const bool live = o < w;
  const float wco = live ? WC[o] : 0.f;
  float acc = 0.f;
  if (live) {
    for (int c = part; c < w; c += 4) acc += wk.dv[c] * WH[(size_t)c * w + o];
    for (int q = part; q < s.NQ; q += 4) acc += wk.Dq[q] * lq[(size_t)q * w + o];
    for (int c = part; c < w; c += 4) dWH[(size_t)c * w + o] += wk.dv[c] * wco;  // rows w..2w of WH see a zero feature
  }
  s_p[part][cl] = acc;
  __syncthreads();
  if (part == 0 && live) {
    const float ds0 = wk.ds0[0];
    dWC[o] += (s_p[0][cl] + s_p[1][cl]) + (s_p[2][cl] + s_p[3][cl]) + ds0 * WHb[o];
    dWHb[o] += ds0 * wco;
    if (o == 0) dWCb[0] += ds0;
  }
}

// ---- the row pass's launch: w -> <TPR, CPT, RPT>, the one table
template <bool TW, bool POOL>
static void shb_launch_rows(const ShShape& s, const ShBwdShape& bs, const ShWork& sv, const ShBwdWork& wk, const float* rows,
                            const float* d_h_a, float* d_rows, const ShBwdTwArgs& ta, hipStream_t st) {
  const dim3 rgrid((unsigned)((int64_t)s.A * s.K * bs.nch));
#define FVTA_SHB_ROWS(TPR, CPT, RPT) \
  hipLaunchKernelGGL((attn_shared_bwd_rows_kernel<TPR, CPT, RPT, TW, POOL>), rgrid, dim3(256), 0, st, s, bs, sv, wk, rows, d_h_a, \
                     d_rows, ta)
  switch (s.w) {
    case 64: FVTA_SHB_ROWS(16, 1, 8); break;
    case 128: FVTA_SHB_ROWS(32, 1, 8); break;
    case 256: FVTA_SHB_ROWS(64, 1, 8); break;
    case 512: FVTA_SHB_ROWS(128, 1, 8); break;
    case 1024: FVTA_SHB_ROWS(256, 1, 8); break;
    default: FVTA_SHB_ROWS(256, 2, 4); break;
  }
#undef FVTA_SHB_ROWS
}

// ---- the question pass's: G = 256 / JP
template <bool TW, bool POOL>
static void shb_launch_q(const ShShape& s, const ShBwdShape& bs, const ShWork& sv, const ShBwdWork& wk, const float* rows,
                         const float* dxs, hipStream_t st) {
  const dim3 qgrid((unsigned)((int64_t)s.ngmax * bs.TS * bs.nsl));
  if (s.G == 8)
    hipLaunchKernelGGL((attn_shared_bwd_q_kernel<8, TW, POOL>), qgrid, dim3(64), 0, st, s, bs, sv, wk, rows, dxs);
  else
    hipLaunchKernelGGL((attn_shared_bwd_q_kernel<4, TW, POOL>), qgrid, dim3(64), 0, st, s, bs, sv, wk, rows, dxs);
}

// ---- the backward driver: the five launches of the header (1 prep, 2 rows, 3 question pass, 4 fold, 5 parameters) for
// fvta_attn_shared_bwd <TW = 0, POOL = 0>, fvta_attn_shared_bwd_tw <1, 0>, fvta_attn_pool_bwd <0, 1> and
// fvta_attn_pool_bwd_tw <1, 1>, with
//   TW    the warp's own kernels (a .. f above) around them, and db left to (e)
//   POOL  3b attn_pool_bwd_dct_kernel in front of the fold, and the pooled fold (attn_pool.hip)
// and both at once: the POOL instantiations of (b) and (c), the rest as it is -- (d) runs over [P,JX]
template <bool TW, bool POOL>
static int shb_backward_as(ShShape s, const char* who, const ShBwdCall& c, const ShBwdWarpCall* warp) {
  hipStream_t st = (hipStream_t)c.stream;
  s.use_mask = (c.rows_mask && c.qmask) ? 1 : 0;
  const ShBwdShape bs = shb_shape(s);
  const ShWork sv(s, const_cast<void*>(c.saved), nullptr);
  const ShBwdTwWork tw(s, bs, c.workspace, POOL);  // (what it carves past `base` is the TW calls' alone: their workspace is larger)
  const ShBwdWork& wk = tw.base;
  ShBwdTwArgs ta{};
  const float* tz = nullptr;
  if constexpr (TW) {
    const ShTwSaved ts(s, sv, const_cast<void*>(c.saved));
    ta = ShBwdTwArgs{ts.scale, ts.lin, ts.r2, tw.ds, tw.dxs, tw.dbt};
    tz = ts.tz;
  }
  ShShape sq = s;  // the prep runs per question over all of its positions
  sq.T = s.TO;
  hipLaunchKernelGGL(attn_shared_bwd_prep_kernel, dim3(s.NQ), dim3(s.K > 4 ? 1024 : 256), 0, st, sq, sv, wk, c.d_h_a);
  if constexpr (TW) hipLaunchKernelGGL(attn_shared_tw_vec_kernel, dim3((s.w + 3) / 4), dim3(256), 0, st, s.w, warp->WH_W, warp->WC_W, tw.v);
  shb_launch_rows<TW, POOL>(s, bs, sv, wk, c.rows, c.d_h_a, c.d_rows, ta, st);
  shb_launch_q<TW, POOL>(s, bs, sv, wk, c.rows, TW ? (const float*)tw.dxs : nullptr, st);
  if constexpr (TW) {
    hipLaunchKernelGGL(attn_shared_bwd_tw_dz_kernel<POOL>, dim3(s.NQ), dim3(256), 0, st, s, (const int*)sv.qslot, warp->warp_type,
                       (int)ceilf(warp->window_t), tz, warp->WC_W, tw, warp->d_lq);
    hipLaunchKernelGGL(attn_shared_bwd_tw_de_kernel<POOL>, dim3(s.A, (s.T + 255) / 256), dim3(256), 0, st, s, sv, tw);
    const dim3 egrid((unsigned)tw.ewg);
    switch (s.w <= 256 ? 1 : s.w / 256) {
      case 1: hipLaunchKernelGGL(attn_shared_bwd_tw_energy_kernel<1>, egrid, dim3(256), 0, st, s, sv, tw, c.rows, c.d_rows); break;
      case 2: hipLaunchKernelGGL(attn_shared_bwd_tw_energy_kernel<2>, egrid, dim3(256), 0, st, s, sv, tw, c.rows, c.d_rows); break;
      case 4: hipLaunchKernelGGL(attn_shared_bwd_tw_energy_kernel<4>, egrid, dim3(256), 0, st, s, sv, tw, c.rows, c.d_rows); break;
      default: hipLaunchKernelGGL(attn_shared_bwd_tw_energy_kernel<8>, egrid, dim3(256), 0, st, s, sv, tw, c.rows, c.d_rows); break;
    }
  }
  const dim3 fgrid(s.NQ, (s.w + 255) / 256, bs.JZ);
  if constexpr (POOL) {
    float* dctq = PoolBwdWork(s, bs, c.workspace).dctq;
    hipLaunchKernelGGL(attn_pool_bwd_dct_kernel, dim3(s.NQ), dim3(64), 0, st, s, bs, sv, wk, dctq);
    hipLaunchKernelGGL(attn_pool_bwd_fold_kernel, fgrid, dim3(256), 0, st, s, bs, sv, wk, (const float*)dctq, c.hq, c.d_hq);
  } else {
    hipLaunchKernelGGL(attn_shared_bwd_fold_kernel, fgrid, dim3(256), 0, st, s, bs, sv, wk, c.hq, c.d_hq);
  }
  // (TW: db is not the sum of the d ct -- the row pass says why; the parameter kernel's bias block adds into nothing)
  hipLaunchKernelGGL(attn_shared_bwd_params_kernel, dim3((s.w + 63) / 64 + 1), dim3(256), 0, st, s, bs, wk, c.dW,
                     TW ? (float*)nullptr : c.db);
  if constexpr (TW) {
    hipLaunchKernelGGL(attn_shared_bwd_tw_dv_kernel, dim3((s.w + 63) / 64 + 1), dim3(256), 0, st, s, tw, c.db);
    hipLaunchKernelGGL(attn_shared_bwd_tw_params_kernel, dim3((s.w + 63) / 64), dim3(256), 0, st, s, tw, warp->WH_W, warp->WH_b,
                       warp->WC_W, warp->lq, warp->dWH_W, warp->dWH_b, warp->dWC_W, warp->dWC_b);
  }
  FVTA_CHECK_LAUNCH(who);
  return FVTA_OK;
}

int shb_backward(const ShShape& s, bool pool, const char* who, const ShBwdCall& c, const ShBwdWarpCall* warp) {
  if (pool) return warp ? shb_backward_as<true, true>(s, who, c, warp) : shb_backward_as<false, true>(s, who, c, nullptr);
  return warp ? shb_backward_as<true, false>(s, who, c, warp) : shb_backward_as<false, false>(s, who, c, nullptr);
}

size_t shb_workspace_bytes(const ShShape& s, bool pool, bool warp) {
  const ShBwdShape b = shb_shape(s);
  if (warp) return ShBwdTwWork(s, b, nullptr, pool).bytes;
  return pool ? PoolBwdWork(s, b, nullptr).bytes : ShBwdWork(s, b, nullptr).bytes;
}

int shb_plan(const ShShape& s, const char* who, int32_t out[4]) {
  FVTA_CHECK_ARG(out != nullptr, "%s: null pointer", who);
  const ShBwdShape b = shb_shape(s);
  out[0] = b.TR;
  out[1] = b.TS;
  out[2] = SHB_CS;
  out[3] = b.tpw;
  return FVTA_OK;
}

}  // namespace fvta
using namespace fvta;

extern "C" size_t fvta_attn_shared_bwd_workspace_bytes(const fvta_attn_shared_desc* d) {
  ShShape s;
  return sh_open(d, "attn_shared_bwd_workspace_bytes", s, SH_BWD) == FVTA_OK ? shb_workspace_bytes(s, false) : 0;
}

extern "C" int fvta_attn_shared_bwd_plan(const fvta_attn_shared_desc* d, int32_t out[4]) {
  ShShape s;
  if (int e = sh_open(d, "attn_shared_bwd_plan", s, SH_BWD)) return e;
  return shb_plan(s, "attn_shared_bwd_plan", out);
}

extern "C" int fvta_attn_shared_bwd(const fvta_attn_shared_desc* d, const float* hinfo, const uint8_t* hmask, const float* hq,
                                    const uint8_t* qmask, const int32_t* album, const float* W, const float* b,
                                    const float* d_h_a, const void* saved, float* d_hinfo, float* d_hq, float* dW, float* db,
                                    void* workspace, fvta_stream_t stream_) {
  ShShape s;
  if (int e = sh_open(d, "attn_shared_bwd", s, SH_BWD)) return e;
  FVTA_CHECK_ARG(hinfo && hq && album && d_h_a && saved && d_hinfo && d_hq && dW && db && workspace,
                 "attn_shared_bwd: null pointer");
  return shb_backward(s, false, "attn_shared_bwd", {hinfo, hmask, hq, qmask, d_h_a, saved, d_hinfo, d_hq, dW, db, workspace, stream_});
}

extern "C" size_t fvta_attn_shared_tw_bwd_workspace_bytes(const fvta_attn_shared_tw_desc* d) {
  ShShape s;
  if (sh_open_tw(d, "attn_shared_tw_bwd_workspace_bytes", s, SH_BWD) != FVTA_OK) return 0;
  return shb_workspace_bytes(s, false, true);
}

extern "C" int fvta_attn_shared_bwd_tw(const fvta_attn_shared_tw_desc* d, const float* hinfo, const uint8_t* hmask, const float* hq,
                                       const uint8_t* qmask, const float* lq, const int32_t* album, const float* W, const float* b,
                                       const float* WH_W, const float* WH_b, const float* WC_W, const float* WC_b,
                                       const float* d_h_a, const void* saved, float* d_hinfo, float* d_hq, float* d_lq, float* dW,
                                       float* db, float* dWH_W, float* dWH_b, float* dWC_W, float* dWC_b, void* workspace,
                                       fvta_stream_t stream_) {
  ShShape s;
  if (int e = sh_open_tw(d, "attn_shared_bwd_tw", s, SH_BWD)) return e;
  FVTA_CHECK_ARG(hinfo && hq && lq && album && W && WH_W && WH_b && WC_W && WC_b && d_h_a && saved && d_hinfo && d_hq && d_lq && dW &&
                     db && dWH_W && dWH_b && dWC_W && dWC_b && workspace,
                 "attn_shared_bwd_tw: null pointer");
  const ShBwdWarpCall warp{d->warp_type, d->window_t, lq, WH_W, WH_b, WC_W, WC_b, d_lq, dWH_W, dWH_b, dWC_W, dWC_b};
  return shb_backward(s, false, "attn_shared_bwd_tw", {hinfo, hmask, hq, qmask, d_h_a, saved, d_hinfo, d_hq, dW, db, workspace, stream_},
                      &warp);
}
