// Focal attention forward for MANY QUESTIONS OVER ONE ALBUM (fvta_attn_shared_fwd): hinfo [A,K,T,w] holds each album's
// context rows once, question i reads album[i]'s.  Per question the result is fvta_attn_fwd's on the pair
// (hinfo[album[i]], hq[i]) -- model_v2.py:210-298 -- but a row is fetched once per GROUP of up to G questions of the same
// album instead of once per question, and the logits of a group are one [rows, w] x [w, G JP] product on the fp32 matrix
// pipe (gemm_f32.h: v_mfma_f32_32x32x2_f32, exact fp32).  No shadow rows; the time warp: fvta_attn_shared_fwd_tw, the TW
// instantiations of (4) and (6), further down.  fvta_attn_shared_fwd keeps nothing
// for a backward; fvta_attn_shared_fwd_train runs the same kernels -- the same bits -- with the ordered plan (3) and the
// arg-max (4) compiled in, and leaves what attn_shared_bwd.hip reads in the caller-held `saved` (attn_shared_common.h).
// fvta_attn_shared_fwd_tw_train is that under the time warp: <TRAIN, TW> of (4), which also leaves lin at the arg-max and r2.
//
// Bilinear form (attn_common.h): x[t,(g,j)] = rs[t] sum_c h[t,c] Qs[g,j,c] + (Rh.h[t] + R2.h[t]^2) + ct[g,j].
// Launches, all on the caller's stream, none waits for the host:
//   1. attn_vecs_kernel            the per-channel vectors of att_logits/W (attn_fwd.hip's)
//   2. attn_shared_prep_q_kernel   Qs [NQ][JP][w] (rows j >= JQ zero), ct [NQ][JP]; JP = 32 (JQ <= 32) or 64
//   3. attn_shared_plan_kernel     one workgroup: counting sort of `album` (clamped into [0, A)), groups of <= G questions
//                                  cut per album: grp[] = {album, first, count}, order[], qslot[], ngroups
//   4. attn_shared_logits_kernel   one workgroup per (group, k, tile of SH_R rows): the product (BM x BN 256 = G JP), row
//                                  terms, tanh, exp_mask, max over j -> amax [NQ,K,T] (and a_logits).  A tile without a
//                                  valid row skips the product: its logits are -1e30 whatever the rows hold
//   5. attn_shared_softmax_kernel  per question: M[k] = max_t amax, L[k] = sum_t exp(amax - M[k]), coef[k] =
//                                  softmax_k(M)[k] / L[k].  Masking needs no special case: a fully masked (album, k) or
//                                  question has amax = -1e30 everywhere, which IS the uniform softmax over all T
//   6. attn_shared_wsum_kernel     one workgroup per (group, k, split of T): part[g] = coef sum_t exp(amax - M) h[t] for
//                                  the G questions from ONE read of each row
//   7. attn_shared_merge_kernel    h_a[q] = sum over (k, split) of the partials, in that order
// Row traffic: (4) and (6) read each row of an album once per group of that album: twice per group, never per question.
// Determinism: no floating-point atomics.  The split of T depends on the descriptor only; a question's numbers do not
// depend on which group, slot or wave it lands in (every column of the product is its own k-ordered fmaf chain, every
// question has its own accumulators), so the integer atomics that place the questions in `order` cannot change a bit.
// The backward DOES sum over an album's questions in `order`: the training plan fills it by ascending question index from a
// single wave (attn_shared_plan_kernel<true>), a function of `album` alone.
#include "attn_shared_common.h"
#include "gemm_f32.h"
#include "timewarp_common.h"

namespace fvta {

// 64 rows x 256 columns, a wave 64 x 64: 200 registers, two workgroups per CU.  (MmaF32<2, 2, 2, 4>, 128 rows and half the
// question staging per row, was measured: 331 registers, one wave per SIMD, and no faster at 8 questions per album, 20 %
// slower at one -- DESIGN.md 4.1)
typedef MmaF32<1, 4, 2, 2> ShMma;
static_assert(ShMma::BM == SH_R && ShMma::BN == SH_BN && ShMma::NT == SH_NT && ShMma::TN % 2 == 0, "tile shape");

// ---- question side.  grid (NQ, JP / 4), 256 threads: a wave per position j
__global__ __launch_bounds__(256) void attn_shared_prep_q_kernel(ShShape s, ShWork wk, const float* __restrict__ hq,
                                                                 const float* __restrict__ bptr) {
  const int q = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, w = s.w;
  const float* Uv = wk.vecs + VEC_U * w;
  const float* Cq = wk.vecs + VEC_CQ * w;
  const float* C2 = wk.vecs + VEC_C2 * w;
  const float bias = (s.simi == 4 || bptr == nullptr) ? 0.f : bptr[0];
  const int j = 4 * blockIdx.y + wave;
  float* dst = wk.Qs + ((size_t)q * s.JP + j) * w;
  if (j >= s.JQ) {  // (wave-uniform)
    for (int c = lane; c < w; c += 64) dst[c] = 0.f;
    if (lane == 0) wk.ct[(size_t)q * s.JP + j] = 0.f;
    return;
  }
  const float* row = hq + ((size_t)q * s.JQ + j) * w;
  float s1 = 0.f, s2 = 0.f;
  for (int c = lane; c < w; c += 64) {
    const float v = row[c];
    s1 += Cq[c] * v + C2[c] * v * v;
    s2 += v * v;
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  const float rq = rsqrtf(fmaxf(s2, 1e-12f));  // tf.nn.l2_normalize eps (cosine only)
  for (int c = lane; c < w; c += 64) dst[c] = s.simi == 4 ? row[c] * rq : row[c] * Uv[c];
  if (lane == 0) wk.ct[(size_t)q * s.JP + j] = s.simi == 4 ? 0.f : s1 + bias;
}

// ---- the plan.  One workgroup.  Indices are data: clamped before they address anything.
__device__ __forceinline__ int sh_album(const int* album, int i, int A) {
  const int a = album[i];
  return a < 0 ? 0 : (a >= A ? A - 1 : a);
}
// ORDERED (the training plan): the questions of an album stand in `order` by ascending question index, so that the
// backward's sum over an album's questions has ONE order, a function of `album` alone.  The cursor atomics below place a
// question wherever its atomic happens to arrive; here wave 0 alone walks the questions 64 at a time in ascending order,
// and per distinct album of a batch ONE lane advances that album's cursor by the number of the batch's questions about
// it, which take their places by lane rank.  Every cursor update is issued by a single wave in program order, one after
// the other: nothing depends on the order in which atomics of different waves arrive.  (An integer atomic is still the
// instruction, because it reads the cursor at L2, past this wave's own vector cache.)
template <bool ORDERED>
__global__ __launch_bounds__(SH_PLAN_NT) void attn_shared_plan_kernel(ShShape s, ShWork wk, const int* __restrict__ album) {
  __shared__ int cell_c[SH_PLAN_NT], cell_g[SH_PLAN_NT];
  const int tid = threadIdx.x, A = s.A, NQ = s.NQ, G = s.G;
  for (int a = tid; a < A; a += SH_PLAN_NT) wk.acnt[a] = 0;
  __syncthreads();
  for (int i = tid; i < NQ; i += SH_PLAN_NT) atomicAdd(&wk.acnt[sh_album(album, i, A)], 1);
  __syncthreads();
  const int C = (A + SH_PLAN_NT - 1) / SH_PLAN_NT;
  const int lo = min(tid * C, A), hi = min(lo + C, A);
  int mine_c = 0, mine_g = 0;
  for (int a = lo; a < hi; ++a) {
    const int c = wk.acnt[a];
    mine_c += c;
    mine_g += (c + G - 1) / G;
  }
  cell_c[tid] = mine_c;
  cell_g[tid] = mine_g;
  __syncthreads();
  for (int o = 1; o < SH_PLAN_NT; o <<= 1) {  // inclusive scans of the chunk sums
    const int vc = tid >= o ? cell_c[tid - o] : 0, vg = tid >= o ? cell_g[tid - o] : 0;
    __syncthreads();
    cell_c[tid] += vc;
    cell_g[tid] += vg;
    __syncthreads();
  }
  int run_c = cell_c[tid] - mine_c, run_g = cell_g[tid] - mine_g;
  for (int a = lo; a < hi; ++a) {
    const int c = wk.acnt[a], ng = (c + G - 1) / G;
    wk.astart[a] = run_c;
    wk.agrp[a] = run_g;
    wk.acnt[a] = 0;  // from here on the album's cursor
    for (int x = 0; x < ng; ++x)
      if (run_g + x < s.ngmax) wk.grp[run_g + x] = int4{a, run_c + x * G, min(G, c - x * G), 0};
    run_c += c;
    run_g += ng;
  }
  if (tid == SH_PLAN_NT - 1) *wk.ngroups = min(cell_g[tid], s.ngmax);
  __syncthreads();
  if constexpr (ORDERED) {
    if (tid >= 64) return;
    for (int base = 0; base < NQ; base += 64) {
      const int i = base + tid;
      const bool ok = i < NQ;
      const int a = ok ? sh_album(album, i, A) : -1;
      unsigned long long todo = __ballot(ok);
      while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int av = __shfl(a, leader, 64);
        const unsigned long long same = __ballot(ok && a == av);
        int first = 0;
        if (tid == leader) first = atomicAdd(&wk.acnt[av], __popcll(same));
        first = __shfl(first, leader, 64);
        if (ok && a == av) {
          const int off = first + __popcll(same & ((1ull << tid) - 1ull));
          wk.order[wk.astart[a] + off] = i;
          wk.qslot[i] = (wk.agrp[a] + off / G) * G + off % G;
        }
        todo &= ~same;
      }
    }
  } else {
    for (int i = tid; i < NQ; i += SH_PLAN_NT) {
      const int a = sh_album(album, i, A);
      const int off = atomicAdd(&wk.acnt[a], 1);
      wk.order[wk.astart[a] + off] = i;
      wk.qslot[i] = (wk.agrp[a] + off / G) * G + off % G;
    }
  }
}

// ---- logits.  grid ngmax * K * ntile, 256 threads
// TRAIN: also the FIRST arg-max j of every row's maximum -> jmax [NQ,K,T] (compile-time: the inference kernel is unchanged)
// TW (compile-time too; tw_scale [NQ,T], else unused): the logits of the WARPED rows h' = s h, s = tw_scale[q,t], from the
// rows as they are held.  The scalar goes through the bilinear form: x = s (h.Qs + Rh.h) + s^2 (R2.h^2) + ct, cosine
// x = (h.Qn) s rsqrt(max(s^2 |h|^2, 1e-12)) -- the row pass keeps Rh.h and R2.h^2 (cosine: the raw sum h^2) apart, and
// the scales of the tile's rows for the group's questions are staged in LDS
template <int JT, bool TRAIN, bool TW>
__global__ __launch_bounds__(SH_NT) void attn_shared_logits_kernel(ShShape s, ShWork wk, const float* __restrict__ hinfo,
                                                                  const uint8_t* __restrict__ hmask,
                                                                  const uint8_t* __restrict__ qmask,
                                                                  float* __restrict__ a_logits, ShTwArgs tw) {
  constexpr int JP = 32 * JT, G = SH_BN / JP;
  const float* __restrict__ tw_scale = tw.scale;
  __shared__ __attribute__((aligned(16))) float smem[ShMma::LDS_FLOATS];
  __shared__ float s_rt[SH_R], s_ct[SH_BN];
  // TW: s_rt holds Rh.h, s_r2 R2.h^2 (cosine: sum h^2); s_sc, s_s2 the factor of the product and the addend per (question, row)
  __shared__ float s_r2[TW ? SH_R : 1], s_sc[TW ? G : 1][TW ? SH_R : 1], s_s2[TW ? G : 1][TW ? SH_R : 1];
  __shared__ int s_q[G];
  __shared__ uint8_t s_hv[SH_R], s_cv[SH_BN];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int tile = blockIdx.x % s.ntile, k = (blockIdx.x / s.ntile) % s.K, grp = blockIdx.x / (s.ntile * s.K);
  if (grp >= *wk.ngroups) return;
  const int4 gi = wk.grp[grp];
  const int a = gi.x, first = gi.y, cnt = gi.z;
  const int T = s.T, w = s.w, JQ = s.JQ, K = s.K, t0 = tile * SH_R;
  const size_t ak = (size_t)a * K + k;
  if (tid < G) s_q[tid] = tid < cnt ? wk.order[first + tid] : -1;
  bool rowv = false;
  if (tid < SH_R) {
    const int t = t0 + tid;
    rowv = t < T && (!s.use_mask || hmask[ak * T + t] != 0);
    s_hv[tid] = rowv;
  }
  __syncthreads();
  {
    const int q = s_q[tid / JP], j = tid % JP;
    const bool ok = q >= 0 && j < JQ;
    s_ct[tid] = ok ? wk.ct[(size_t)q * JP + j] : 0.f;
    s_cv[tid] = ok && (!s.use_mask || qmask[(size_t)q * JQ + j] != 0);
  }
  const int anyrow = __syncthreads_or(rowv ? 1 : 0);
  if (!anyrow) {  // every logit of the tile is masked: -1e30, whatever the rows hold
    const int rows = min(SH_R, T - t0);
    for (int e = tid; e < cnt * rows; e += SH_NT) {
      const size_t at = ((size_t)s_q[e / rows] * K + k) * T + t0 + e % rows;
      wk.amax[at] = FVTA_NEG;
      if constexpr (TRAIN) wk.jmax[at] = 0;
      if constexpr (TRAIN && TW) tw.lin[at] = 0.f;  // (no gradient passes through a masked logit: written, never used)
    }
    if constexpr (TRAIN && TW)
      if (grp == wk.agrp[a])
        for (int e = tid; e < rows; e += SH_NT) tw.r2[ak * T + t0 + e] = 0.f;
    if (a_logits)
      for (int g = 0; g < cnt; ++g) {
        float* dst = a_logits + (((size_t)s_q[g] * K + k) * T + t0) * JQ;
        for (int e = tid; e < rows * JQ; e += SH_NT) dst[e] = FVTA_NEG;
      }
    return;
  }
  const float* hbase = hinfo + ak * T * w;
  // row terms: a wave per SH_R / 4 rows.  cosine: 1 / |h| instead
  {
    const float* Rh = wk.vecs + VEC_RH * w;
    const float* R2 = wk.vecs + VEC_R2 * w;
    for (int r = wave * (SH_R / 4); r < (wave + 1) * (SH_R / 4); ++r) {
      const int t = t0 + r;
      float acc = 0.f;
      if constexpr (TW) {
        float acc2 = 0.f;
        if (t < T)
          for (int c = 4 * lane; c < w; c += 256) {
            const f32x4 h = ld4(hbase + (size_t)t * w + c);
            const f32x4 v1 = h * ld4(Rh + c), v2 = h * h * ld4(R2 + c);
            acc += (v1[0] + v1[1]) + (v1[2] + v1[3]);
            acc2 += (v2[0] + v2[1]) + (v2[2] + v2[3]);
          }
        acc = wave_sum(acc);
        acc2 = wave_sum(acc2);
        if (lane == 0) {
          s_rt[r] = acc;
          s_r2[r] = acc2;
        }
      } else {
        if (t < T)
          for (int c = 4 * lane; c < w; c += 256) {
            const f32x4 h = ld4(hbase + (size_t)t * w + c);
            const f32x4 v = h * (ld4(Rh + c) + ld4(R2 + c) * h);
            acc += (v[0] + v[1]) + (v[2] + v[3]);
          }
        acc = wave_sum(acc);
        if (lane == 0) s_rt[r] = s.simi == 4 ? rsqrtf(fmaxf(acc, 1e-12f)) : acc;
      }
    }
    if constexpr (TW)  // the scales of the tile's rows, per question of the group (an empty slot, a row past T: 0)
      for (int e = tid; e < G * SH_R; e += SH_NT) {
        const int q = s_q[e / SH_R], t = t0 + e % SH_R;
        s_sc[e / SH_R][e % SH_R] = (q >= 0 && t < T) ? tw_scale[(size_t)q * T + t] : 0.f;
      }
  }
  ShMma mma;
  mma.init(tid);
  StageKContig<SH_R, ShMma::BK, SH_NT, ShMma::LDA> sa;
  StageKContig<SH_BN, ShMma::BK, SH_NT, ShMma::LDB> sb;
  auto fa = [&](int r, int kk, bool& ok) -> const float* {
    const int t = t0 + r;
    ok = t < T;
    return hbase + (ok ? (size_t)t * w + kk : (size_t)0);
  };
  const float* Qs = wk.Qs;
  auto fb = [&](int c, int kk, bool& ok) -> const float* {
    const int q = s_q[c / JP];
    ok = q >= 0;
    return Qs + (ok ? ((size_t)q * JP + c % JP) * w + kk : (size_t)0);
  };
  gemm_mainloop(mma, sa, sb, fa, fb, 0, w, smem, tid);  // (ends on a barrier: s_rt -- TW: s_r2, s_sc -- is visible)
  if constexpr (TRAIN && TW) {  // r2 [A,K,T] for the backward: every group of the album holds the same bits, its first stores
    if (grp == wk.agrp[a])
      for (int e = tid; e < min(SH_R, T - t0); e += SH_NT) tw.r2[ak * T + t0 + e] = s_r2[e];
  }
  if constexpr (TW) {  // x = sc (h.Qs + Rh.h) + sc^2 R2.h^2 + ct; cosine (Rh.h = ct = 0): x = h.Qn sc rsqrt(max(sc^2 |h|^2, 1e-12))
    for (int e = tid; e < G * SH_R; e += SH_NT) {
      const float sc = s_sc[e / SH_R][e % SH_R], r2 = sc * sc * s_r2[e % SH_R];
      s_sc[e / SH_R][e % SH_R] = s.simi == 4 ? sc * rsqrtf(fmaxf(r2, 1e-12f)) : sc;
      s_s2[e / SH_R][e % SH_R] = s.simi == 4 ? 0.f : r2;
    }
    __syncthreads();
  }
  // epilogue.  A wave holds TM x TN tiles of 32 x 32: JT = 1: a question per column tile; JT = 2: one per pair of them
  const bool cosine = s.simi == 4, tanh_on = s.add_tanh && !cosine;
#pragma unroll
  for (int i = 0; i < ShMma::TM; ++i) {
    float mx[ShMma::TN][16];
#pragma unroll
    for (int jn = 0; jn < ShMma::TN; ++jn) {
      const int col = mma.col_of(jn), q = s_q[col / JP], j = col % JP;
      const bool colv = s_cv[col] != 0, live = q >= 0 && j < JQ;
      const float ctv = s_ct[col];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = mma.row_of(i, r), t = t0 + row;
        float x = mma.acc[i][jn][r];
        if constexpr (TW) {
          x = s_sc[col / JP][row] * (x + s_rt[row]) + s_s2[col / JP][row] + ctv;
        } else {
          x = cosine ? x * s_rt[row] : x + s_rt[row] + ctv;
        }
        if (tanh_on) x = tanhf(x);
        const float v = (colv && s_hv[row]) ? x : FVTA_NEG;  // exp_mask: x + -1e30 is -1e30 in fp32
        if (a_logits && live && t < T) a_logits[(((size_t)q * K + k) * T + t) * JQ + j] = v;
        mx[jn][r] = live ? v : -INFINITY;
      }
    }
#pragma unroll
    for (int jn = 0; jn < ShMma::TN; jn += JT) {
      const int q = s_q[mma.col_of(jn) / JP];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float m = JT == 2 ? fmaxf(mx[jn][r], mx[jn + 1][r]) : mx[jn][r];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));  // over the 32 columns, rows stay apart
        const int t = t0 + mma.row_of(i, r);
        if (mma.l31 == r && q >= 0 && t < T) wk.amax[((size_t)q * K + k) * T + t] = m;
        if constexpr (TRAIN) {  // columns of a lane: j = l31 (and 32 + l31); a dead column holds -inf and never equals m
          int jm = mx[jn][r] == m ? mma.l31 : 255;
          if (JT == 2 && jm == 255 && mx[jn + 1][r] == m) jm = 32 + mma.l31;
#pragma unroll
          for (int o = 16; o > 0; o >>= 1) jm = min(jm, __shfl_xor(jm, o, 64));
          if (mma.l31 == r && q >= 0 && t < T) wk.jmax[((size_t)q * K + k) * T + t] = (uint8_t)min(jm, JQ - 1);
          if constexpr (TW) {  // lin at the winner: the one lane that holds column jm puts it in, 31 zeros are added to it
            const int mine = mx[jn][r] == m ? mma.l31 : ((JT == 2 && mx[jn + 1][r] == m) ? 32 + mma.l31 : 255);
            const float acc = (JT == 2 && mine >= 32) ? mma.acc[i][JT == 2 ? jn + 1 : jn][r] : mma.acc[i][jn][r];
            float lv = (mine == jm && jm != 255) ? acc + s_rt[mma.row_of(i, r)] : 0.f;
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) lv += __shfl_xor(lv, o, 64);
            if (mma.l31 == r && q >= 0 && t < T) tw.lin[((size_t)q * K + k) * T + t] = lv;
          }
        }
      }
    }
  }
}

// the same bits in every thread: butterflies inside a wave, the four wave results in order
__device__ __forceinline__ float sh_block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ __forceinline__ float sh_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- the two softmaxes' scalars.  grid NQ, 256 threads, K <= 64
__global__ __launch_bounds__(256) void attn_shared_softmax_kernel(ShShape s, ShWork wk) {
  __shared__ float red[4], s_M[64], s_L[64];
  const int q = blockIdx.x, tid = threadIdx.x, T = s.T, K = s.K;
  for (int k = 0; k < K; ++k) {
    const float* am = wk.amax + ((size_t)q * K + k) * T;
    float m = -INFINITY;
    for (int t = tid; t < T; t += 256) m = fmaxf(m, am[t]);
    m = sh_block_max(m, red);
    float l = 0.f;
    for (int t = tid; t < T; t += 256) l += expf(am[t] - m);
    l = sh_block_sum(l, red);
    if (tid == 0) {
      s_M[k] = m;
      s_L[k] = l;
    }
  }
  __syncthreads();
  if (tid == 0) {  // outer softsel over K (model_v2.py:278): logits = max over (t, j) of the masked logits
    float mx = -INFINITY, sum = 0.f;
    for (int k = 0; k < K; ++k) mx = fmaxf(mx, s_M[k]);
    for (int k = 0; k < K; ++k) sum += expf(s_M[k] - mx);
    for (int k = 0; k < K; ++k) {
      wk.M[(size_t)q * K + k] = s_M[k];
      wk.coef[(size_t)q * K + k] = expf(s_M[k] - mx) / sum / s_L[k];
      if (wk.L) {  // training: the two factors of coef, apart
        wk.L[(size_t)q * K + k] = s_L[k];
        wk.r[(size_t)q * K + k] = expf(s_M[k] - mx) / sum;
      }
    }
  }
}

// ---- weighted sums.  grid ngmax * K * S, 256 threads: thread tid owns channels 4 tid .. + 3 (+ 1024 per further CPT)
// TW (compile-time; tw_scale [NQ,T], else unused): the sum runs over the warped rows s h: the staged weight carries s
template <int G, int CPT, bool TW>
__global__ __launch_bounds__(256) void attn_shared_wsum_kernel(ShShape s, ShWork wk, const float* __restrict__ hinfo,
                                                               const float* __restrict__ tw_scale) {
  __shared__ float s_p[SH_CH][G], s_M[G], s_cf[G];
  __shared__ int s_q[G];
  const int tid = threadIdx.x;
  const int sp = blockIdx.x % s.S, k = (blockIdx.x / s.S) % s.K, grp = blockIdx.x / (s.S * s.K);
  if (grp >= *wk.ngroups) return;
  const int4 gi = wk.grp[grp];
  const int a = gi.x, first = gi.y, cnt = gi.z;
  const int T = s.T, w = s.w, K = s.K;
  if (tid < G) {
    const int q = tid < cnt ? wk.order[first + tid] : -1;
    s_q[tid] = q;
    s_M[tid] = q >= 0 ? wk.M[(size_t)q * K + k] : 0.f;
    s_cf[tid] = q >= 0 ? wk.coef[(size_t)q * K + k] : 0.f;
  }
  f32x4 acc[G][CPT];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int i = 0; i < CPT; ++i) acc[g][i] = zero4();
  const int tb = sp * s.rps, te = min(T, tb + s.rps);
  const float* hbase = hinfo + ((size_t)a * K + k) * T * w;
  const bool mine = 4 * tid < w;
  for (int c0 = tb; c0 < te; c0 += SH_CH) {
    __syncthreads();
    for (int e = tid; e < SH_CH * G; e += 256) {
      const int g = e / SH_CH, r = e % SH_CH, t = c0 + r, q = s_q[g];
      float p = (t < te && q >= 0) ? expf(wk.amax[((size_t)q * K + k) * T + t] - s_M[g]) : 0.f;
      if constexpr (TW) p = (t < te && q >= 0) ? p * tw_scale[(size_t)q * T + t] : 0.f;
      s_p[r][g] = p;
    }
    __syncthreads();
    const int nr = min(SH_CH, te - c0);
    if (mine) {
#pragma unroll 4
      for (int r = 0; r < nr; ++r) {
        const float* row = hbase + (size_t)(c0 + r) * w + 4 * tid;
        f32x4 h[CPT];
#pragma unroll
        for (int i = 0; i < CPT; ++i) h[i] = ld4(row + 1024 * i);
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float p = s_p[r][g];
#pragma unroll
          for (int i = 0; i < CPT; ++i) acc[g][i] += h[i] * p;
        }
      }
    }
  }
  if (mine) {
    float* dst = wk.part + (((size_t)grp * K + k) * s.S + sp) * G * w + 4 * tid;
#pragma unroll
    for (int g = 0; g < G; ++g)
      if (g < cnt) {
        const float cf = s_cf[g];
#pragma unroll
        for (int i = 0; i < CPT; ++i) *reinterpret_cast<f32x4*>(dst + (size_t)g * w + 1024 * i) = acc[g][i] * cf;
      }
  }
}

// ---- merge.  grid (NQ, ceil(w / 256)): a channel per thread, the partials in (k, split) order
__global__ __launch_bounds__(256) void attn_shared_merge_kernel(ShShape s, ShWork wk, float* __restrict__ h_a) {
  const int q = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
  if (c >= s.w) return;
  const int slot = wk.qslot[q], grp = slot / s.G, g = slot % s.G;
  float v = 0.f;
  for (int k = 0; k < s.K; ++k) {
    float vk = 0.f;  // training: r[k] u[k], beside h_a's own chain (whose order of sums stays what it is)
    for (int sp = 0; sp < s.S; ++sp) {
      const float p = wk.part[((((size_t)grp * s.K + k) * s.S + sp) * s.G + g) * s.w + c];
      v += p;
      vk += p;
    }
    if (wk.u) {  // r = 0 (underflow): u[k] reaches nothing in the backward, every use carries a factor r
      const float r = wk.r[(size_t)q * s.K + k];
      wk.u[((size_t)q * s.K + k) * s.w + c] = r > 0.f ? vk / r : 0.f;
    }
  }
  h_a[(size_t)q * s.w + c] = v;
}

// ---- under the time warp (fvta_attn_shared_fwd_tw).  The warp (timewarp.hip) is one scalar per (question, position):
//   h'[q,k,t,:] = h[a,k,t,:] scale[q,t],   scale[q,t] = tanh(e[a,t] + K (s0 + WC . lq[q])) cnt(t),   a = album[q]
//   e[a,t] = sum_k sum_c v[c] h[a,k,t,c]^2,   v = WH[:w] WC,   s0 = b_WH . WC + b_WC
// and only e reads the rows: it belongs to the album and is computed once per album set (fvta_attn_shared_energy).
// v[c] = sum_o WH[c][o] WC[o]: tw_vec_kernel's arithmetic (a wave per output, lane-strided, wave_sum).  grid w / 4
__global__ __launch_bounds__(256) void attn_shared_tw_vec_kernel(int w, const float* __restrict__ WH, const float* __restrict__ WC,
                                                                 float* __restrict__ v) {
  const int o = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (o >= w) return;
  float acc = 0.f;
  for (int c = lane; c < w; c += 64) acc += WH[(size_t)o * w + c] * WC[c];
  acc = wave_sum(acc);
  if (lane == 0) v[o] = acc;
}

// e[a,t]: a wave per (a, t), every k (masked rows included, as tw_coef_kernel), in tw_coef_kernel's order.  grid ceil(A T / 4)
__global__ __launch_bounds__(256) void attn_shared_energy_kernel(ShShape s, const float* __restrict__ hinfo, const float* __restrict__ v,
                                                                 float* __restrict__ energy) {
  const int64_t pos = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (pos >= (int64_t)s.A * s.T) return;
  const int a = (int)(pos / s.T), t = (int)(pos % s.T);
  float acc = 0.f;
  for (int k = 0; k < s.K; ++k) {
    const float* row = hinfo + (((size_t)a * s.K + k) * s.T + t) * s.w;
    for (int c = lane * 4; c < s.w; c += 256) {
      const f32x4 h = ld4(row + c), vv = ld4(v + c);
      const f32x4 p = h * h * vv;
      acc += (p[0] + p[1]) + (p[2] + p[3]);
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) energy[pos] = acc;
}

// scale[q,t].  grid (NQ, ceil(T / 256)), 256 threads; every wave takes the two dot products itself (w floats each)
// TRAIN: tanh(z) beside it, for the backward
template <bool TRAIN>
__global__ __launch_bounds__(256) void attn_shared_tw_scale_kernel(ShShape s, int warp_type, int win, const float* __restrict__ energy,
                                                                   const float* __restrict__ lq, const int* __restrict__ album,
                                                                   const float* __restrict__ WHb, const float* __restrict__ WC,
                                                                   const float* __restrict__ WCb, float* __restrict__ scale,
                                                                   float* __restrict__ scale_out, float* __restrict__ tz_out) {
  const int q = blockIdx.x, lane = threadIdx.x & 63, t = blockIdx.y * 256 + threadIdx.x;
  float s0 = 0.f, sq = 0.f;
  for (int c = lane; c < s.w; c += 64) {
    const float wc = WC[c];
    s0 += WHb[c] * wc;
    sq += lq[(size_t)q * s.w + c] * wc;
  }
  s0 = wave_sum(s0) + WCb[0];
  sq = wave_sum(sq);
  if (t >= s.T) return;
  const int a = sh_album(album, q, s.A);
  const float tz = tanhf(energy[(size_t)a * s.T + t] + (float)s.K * (s0 + sq));
  const float sc = tz * tw_count(t, s.T, warp_type, win);
  if constexpr (TRAIN) tz_out[(size_t)q * s.T + t] = tz;
  scale[(size_t)q * s.T + t] = sc;
  if (scale_out) scale_out[(size_t)q * s.T + t] = sc;
}

// 0: fine, else the status with the message set
int fvta_attn_shared_check(const fvta_attn_shared_desc* d, const char* who) {
  FVTA_CHECK_ARG(d != nullptr, "%s: null descriptor", who);
  FVTA_CHECK_ARG(d->A > 0 && d->NQ > 0 && d->K > 0 && d->T > 0 && d->JQ > 0 && d->w > 0, "%s: bad A/NQ/K/T/JQ/w (%d,%d,%d,%d,%d,%d)",
                 who, d->A, d->NQ, d->K, d->T, d->JQ, d->w);
  const char* why = nullptr;
  const int w = d->w;
  if (d->simi < 1 || d->simi > 4) {
    fvta_set_error("%s: similarity matrix not implemented (simiMatrix=%d)", who, d->simi);
    return FVTA_ERR_UNSUPPORTED;
  }
  if (!(w == 64 || w == 128 || w == 256 || w == 512 || w == 1024 || w == 2048))
    why = "w must be one of 64,128,256,512,1024,2048";
  else if (d->JQ > 64)
    why = "JQ must be 1..64";
  else if (d->K > 64)
    why = "K must be 1..64";
  else if (d->A > (1 << 28) || d->NQ > (1 << 28))
    why = "A and NQ must not exceed 2^28";
  if (!why) {
    const ShShape s = sh_shape(d);
    if ((int64_t)s.ngmax * d->K * s.ntile > 0x7fffffff || (int64_t)s.ngmax * d->K * s.S > 0x7fffffff) why = "too many workgroups";
  }
  if (why) {
    fvta_set_error("%s: unsupported shape (A=%d NQ=%d K=%d T=%d JQ=%d w=%d): %s", who, d->A, d->NQ, d->K, d->T, d->JQ, w, why);
    return FVTA_ERR_UNSUPPORTED;
  }
  return FVTA_OK;
}

template <int G, bool TW>
static void sh_launch_wsum(const ShShape& s, const ShWork& wk, const float* hinfo, const float* tw_scale, hipStream_t st) {
  const dim3 grid((unsigned)((int64_t)s.ngmax * s.K * s.S));
  if (s.w <= 1024)
    hipLaunchKernelGGL((attn_shared_wsum_kernel<G, 1, TW>), grid, dim3(256), 0, st, s, wk, hinfo, tw_scale);
  else
    hipLaunchKernelGGL((attn_shared_wsum_kernel<G, 2, TW>), grid, dim3(256), 0, st, s, wk, hinfo, tw_scale);
}

}  // namespace fvta
using namespace fvta;

extern "C" size_t fvta_attn_shared_workspace_bytes(const fvta_attn_shared_desc* d) {
  if (fvta_attn_shared_check(d, "attn_shared_workspace_bytes") != FVTA_OK) return 0;
  return ShWork(sh_shape(d), nullptr).bytes;
}

extern "C" int fvta_attn_shared_plan(const fvta_attn_shared_desc* d, int32_t out[4]) {
  if (int e = fvta_attn_shared_check(d, "attn_shared_plan")) return e;
  FVTA_CHECK_ARG(out != nullptr, "attn_shared_plan: null pointer");
  const ShShape s = sh_shape(d);
  out[0] = s.G;
  out[1] = SH_R;
  out[2] = s.S;
  out[3] = s.rps;
  return FVTA_OK;
}

// the seven launches; TRAIN: the ordered plan and the arg-max, wk carved from (saved, workspace); TW: under the time warp,
// tw_scale [NQ,T] written by an earlier launch on the same stream
template <bool TRAIN, bool TW = false>
static int sh_forward(ShShape s, const ShWork& wk, const float* hinfo, const uint8_t* hmask, const float* hq, const uint8_t* qmask,
                      const int32_t* album, const float* W, const float* b, float* h_a, float* a_logits, hipStream_t st,
                      const float* tw_scale = nullptr, const char* who = nullptr, float* tw_lin = nullptr, float* tw_r2 = nullptr) {
  s.use_mask = (hmask && qmask) ? 1 : 0;  // model_v2.py:233: the mask applies only when both are given
  // attn_fwd.hip's kernel, declared in attn_common.h (feat_order 0 = model_v2.py's)
  hipLaunchKernelGGL(attn_vecs_kernel, dim3((s.w + 255) / 256), dim3(256), 0, st, W, s.w, s.simi, 0, wk.vecs);
  hipLaunchKernelGGL(attn_shared_prep_q_kernel, dim3(s.NQ, s.JP / 4), dim3(256), 0, st, s, wk, hq, b);
  hipLaunchKernelGGL(attn_shared_plan_kernel<TRAIN>, dim3(1), dim3(SH_PLAN_NT), 0, st, s, wk, (const int*)album);
  const dim3 lgrid((unsigned)((int64_t)s.ngmax * s.K * s.ntile));
  const ShTwArgs tw{tw_scale, tw_lin, tw_r2};
  if (s.JP == 32)
    hipLaunchKernelGGL((attn_shared_logits_kernel<1, TRAIN, TW>), lgrid, dim3(SH_NT), 0, st, s, wk, hinfo, hmask, qmask, a_logits,
                       tw);
  else
    hipLaunchKernelGGL((attn_shared_logits_kernel<2, TRAIN, TW>), lgrid, dim3(SH_NT), 0, st, s, wk, hinfo, hmask, qmask, a_logits,
                       tw);
  hipLaunchKernelGGL(attn_shared_softmax_kernel, dim3(s.NQ), dim3(256), 0, st, s, wk);
  if (s.G == 8)
    sh_launch_wsum<8, TW>(s, wk, hinfo, tw_scale, st);
  else
    sh_launch_wsum<4, TW>(s, wk, hinfo, tw_scale, st);
  hipLaunchKernelGGL(attn_shared_merge_kernel, dim3(s.NQ, (s.w + 255) / 256), dim3(256), 0, st, s, wk, h_a);
  FVTA_CHECK_LAUNCH(who ? who : (TRAIN ? "attn_shared_fwd_train" : "attn_shared_fwd"));
  return FVTA_OK;
}

extern "C" int fvta_attn_shared_fwd(const fvta_attn_shared_desc* d, const float* hinfo, const uint8_t* hmask, const float* hq,
                                    const uint8_t* qmask, const int32_t* album, const float* W, const float* b, float* h_a,
                                    float* a_logits, void* workspace, fvta_stream_t stream_) {
  if (int e = fvta_attn_shared_check(d, "attn_shared_fwd")) return e;
  FVTA_CHECK_ARG(hinfo && hq && album && h_a && workspace, "attn_shared_fwd: null pointer");
  FVTA_CHECK_ARG(d->simi == 4 || W, "attn_shared_fwd: simiMatrix %d needs att_logits/W", d->simi);
  const ShShape s = sh_shape(d);
  return sh_forward<false>(s, ShWork(s, workspace), hinfo, hmask, hq, qmask, album, W, b, h_a, a_logits, (hipStream_t)stream_);
}

// ---- training.  The same kernels on the same numbers (h_a and a_logits are fvta_attn_shared_fwd's bits: the placement of
// a question changes none, see the header), with what the backward (attn_shared_bwd.hip) reads left in `saved`.
int fvta::fvta_attn_shared_check_train(const fvta_attn_shared_desc* d, const char* who) {
  if (int e = fvta_attn_shared_check(d, who)) return e;
  if (d->simi == 4) {
    fvta_set_error("%s: simiMatrix 4 has no shared-context backward (simiMatrix 1-3); the per-question route "
                   "(fvta_attn_fwd / fvta_attn_bwd on the gathered rows) covers it", who);
    return FVTA_ERR_UNSUPPORTED;
  }
  return FVTA_OK;
}

extern "C" size_t fvta_attn_shared_saved_bytes(const fvta_attn_shared_desc* d) {
  if (fvta_attn_shared_check_train(d, "attn_shared_saved_bytes") != FVTA_OK) return 0;
  return ShWork(sh_shape(d), nullptr, nullptr).saved_bytes;
}

extern "C" int fvta_attn_shared_fwd_train(const fvta_attn_shared_desc* d, const float* hinfo, const uint8_t* hmask,
                                          const float* hq, const uint8_t* qmask, const int32_t* album, const float* W,
                                          const float* b, float* h_a, float* a_logits, void* saved, void* workspace,
                                          fvta_stream_t stream_) {
  if (int e = fvta_attn_shared_check_train(d, "attn_shared_fwd_train")) return e;
  FVTA_CHECK_ARG(hinfo && hq && album && W && h_a && saved && workspace, "attn_shared_fwd_train: null pointer");
  const ShShape s = sh_shape(d);
  return sh_forward<true>(s, ShWork(s, saved, workspace), hinfo, hmask, hq, qmask, album, W, b, h_a, a_logits,
                          (hipStream_t)stream_);
}

// ---- under the time warp.  The workspace: fvta_attn_shared_fwd's, then scale [NQ,T], then v [w] (the energy call's)
namespace fvta {
struct ShTwWork {
  ShWork wk;
  float *scale, *v;
  size_t bytes;
  ShTwWork(const ShShape& s, void* p) : wk(s, p) {
    FvtaCarver c(p);
    c.off = wk.bytes;
    scale = c.take<float>((size_t)s.NQ * s.T);
    v = c.take<float>((size_t)s.w);
    bytes = c.off;
  }
};

int fvta_attn_shared_check_tw(const fvta_attn_shared_tw_desc* d, const char* who, bool train) {
  FVTA_CHECK_ARG(d != nullptr, "%s: null descriptor", who);
  if (int e = train ? fvta_attn_shared_check_train(&d->shape, who) : fvta_attn_shared_check(&d->shape, who)) return e;
  if (d->warp_type < 1 || d->warp_type > 5) {
    fvta_set_error("%s: time warping type not implemented (warp_type=%d)", who, d->warp_type);  // model_v2.py:341
    return FVTA_ERR_INVALID_ARG;
  }
  FVTA_CHECK_ARG(d->window_t >= 0.f && d->window_t <= 1e9f, "%s: bad window_t (%g)", who, (double)d->window_t);
  if (d->shape.T > 65535 * 256) {
    fvta_set_error("%s: unsupported shape (T=%d): T must not exceed 65535 * 256 under the time warp", who, d->shape.T);
    return FVTA_ERR_UNSUPPORTED;
  }
  return FVTA_OK;
}
}  // namespace fvta

extern "C" size_t fvta_attn_shared_tw_workspace_bytes(const fvta_attn_shared_tw_desc* d) {
  if (fvta_attn_shared_check_tw(d, "attn_shared_tw_workspace_bytes") != FVTA_OK) return 0;
  return ShTwWork(sh_shape(&d->shape), nullptr).bytes;
}

extern "C" int fvta_attn_shared_energy(const fvta_attn_shared_tw_desc* d, const float* hinfo, const float* WH_W, const float* WC_W,
                                       float* energy, void* workspace, fvta_stream_t stream_) {
  if (int e = fvta_attn_shared_check_tw(d, "attn_shared_energy")) return e;
  FVTA_CHECK_ARG(hinfo && WH_W && WC_W && energy && workspace, "attn_shared_energy: null pointer");
  const ShShape s = sh_shape(&d->shape);
  const ShTwWork tw(s, workspace);
  hipStream_t st = (hipStream_t)stream_;
  hipLaunchKernelGGL(attn_shared_tw_vec_kernel, dim3((s.w + 3) / 4), dim3(256), 0, st, s.w, WH_W, WC_W, tw.v);
  hipLaunchKernelGGL(attn_shared_energy_kernel, dim3((unsigned)(((int64_t)s.A * s.T + 3) / 4)), dim3(256), 0, st, s, hinfo, tw.v,
                     energy);
  FVTA_CHECK_LAUNCH("attn_shared_energy");
  return FVTA_OK;
}

extern "C" int fvta_attn_shared_fwd_tw(const fvta_attn_shared_tw_desc* d, const float* hinfo, const uint8_t* hmask,
                                       const float* energy, const float* hq, const uint8_t* qmask, const float* lq,
                                       const int32_t* album, const float* W, const float* b, const float* WH_b, const float* WC_W,
                                       const float* WC_b, float* h_a, float* a_logits, float* scale_out, void* workspace,
                                       fvta_stream_t stream_) {
  if (int e = fvta_attn_shared_check_tw(d, "attn_shared_fwd_tw")) return e;
  FVTA_CHECK_ARG(hinfo && energy && hq && lq && album && WH_b && WC_W && WC_b && h_a && workspace, "attn_shared_fwd_tw: null pointer");
  FVTA_CHECK_ARG(d->shape.simi == 4 || W, "attn_shared_fwd_tw: simiMatrix %d needs att_logits/W", d->shape.simi);
  const ShShape s = sh_shape(&d->shape);
  const ShTwWork tw(s, workspace);
  hipStream_t st = (hipStream_t)stream_;
  hipLaunchKernelGGL(attn_shared_tw_scale_kernel<false>, dim3(s.NQ, (s.T + 255) / 256), dim3(256), 0, st, s, d->warp_type,
                     (int)ceilf(d->window_t), energy, lq, (const int*)album, WH_b, WC_W, WC_b, tw.scale, scale_out, (float*)nullptr);
  return sh_forward<false, true>(s, tw.wk, hinfo, hmask, hq, qmask, album, W, b, h_a, a_logits, st, tw.scale, "attn_shared_fwd_tw");
}

// ---- training under the time warp.  The kernels of fvta_attn_shared_fwd_tw on the same numbers -- h_a, a_logits and
// scale_out are its bits -- with the ordered plan, the arg-max, and in `saved` what attn_shared_bwd.hip's
// fvta_attn_shared_bwd_tw reads: fvta_attn_shared_fwd_train's pieces, then scale, tanh(z), lin at the arg-max and r2.
extern "C" size_t fvta_attn_shared_tw_saved_bytes(const fvta_attn_shared_tw_desc* d) {
  if (fvta_attn_shared_check_tw(d, "attn_shared_tw_saved_bytes", true) != FVTA_OK) return 0;
  const ShShape s = sh_shape(&d->shape);
  return ShTwSaved(s, ShWork(s, nullptr, nullptr), nullptr).bytes;
}

extern "C" int fvta_attn_shared_fwd_tw_train(const fvta_attn_shared_tw_desc* d, const float* hinfo, const uint8_t* hmask,
                                             const float* energy, const float* hq, const uint8_t* qmask, const float* lq,
                                             const int32_t* album, const float* W, const float* b, const float* WH_b,
                                             const float* WC_W, const float* WC_b, float* h_a, float* a_logits, float* scale_out,
                                             void* saved, void* workspace, fvta_stream_t stream_) {
  if (int e = fvta_attn_shared_check_tw(d, "attn_shared_fwd_tw_train", true)) return e;
  FVTA_CHECK_ARG(hinfo && energy && hq && lq && album && W && WH_b && WC_W && WC_b && h_a && saved && workspace,
                 "attn_shared_fwd_tw_train: null pointer");
  const ShShape s = sh_shape(&d->shape);
  const ShWork wk(s, saved, workspace);  // (its share of the workspace is no larger than the inference call's)
  const ShTwSaved ts(s, wk, saved);
  hipStream_t st = (hipStream_t)stream_;
  hipLaunchKernelGGL(attn_shared_tw_scale_kernel<true>, dim3(s.NQ, (s.T + 255) / 256), dim3(256), 0, st, s, d->warp_type,
                     (int)ceilf(d->window_t), energy, lq, (const int*)album, WH_b, WC_W, WC_b, ts.scale, scale_out, ts.tz);
  return sh_forward<true, true>(s, wk, hinfo, hmask, hq, qmask, album, W, b, h_a, a_logits, st, ts.scale, "attn_shared_fwd_tw_train",
                                ts.lin, ts.r2);
}
