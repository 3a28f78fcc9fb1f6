// The kernel templates the shared-context forward (attn_shared.hip) and the pooled forward (attn_pool.hip) both
// instantiate: the plan, the logits and the weighted sum.  ONE copy of each; what differs between the two callers is what
// a column block of a group's product stands for, and that is the compile-time flag POOL:
//   POOL = false  a reference IS a question: order[] holds question ids, the question's T positions are the album's rows
//   POOL = true   a reference is a (question, slot) pair, id q * M + m: the block reads question q's Qs / ct / qmask and
//                 writes positions m * T .. + T of q's M * T (s.T = JX, the rows of ONE pooled album; s.TO = M * T).
//                 A negative index is an empty slot: it joins no group and its qslot is -1
// sh_ref_q / sh_ref_off (attn_shared_common.h: the backward's kernels use them too) are the whole of it; with
// POOL = false they fold to (ref, 0) and the kernels are what they were.  The kernels that read rows also take the rows'
// type, ROW: float, or bf16_t for a pool held in bf16 (the fvta_attn_pool_*_bf16 entry points) -- the loads widen, the
// arithmetic is the fp32 kernel's.  The non-template kernels both callers launch
// (question side, the softmaxes' scalars) stay in attn_shared.hip.
#pragma once
#include "attn_shared_common.h"
#include "gemm_f32.h"

namespace fvta {

// attn_shared.hip.  grid (NQ, JP / 4), 256 threads
__global__ __launch_bounds__(256) void attn_shared_prep_q_kernel(ShShape s, ShWork wk, const float* __restrict__ hq,
                                                                 const float* __restrict__ bptr);
// attn_shared.hip.  grid NQ, 256 threads: over s.T positions per (question, k) -- the pooled caller passes T = M * JX
__global__ __launch_bounds__(256) void attn_shared_softmax_kernel(ShShape s, ShWork wk);

// 64 rows x 256 columns, a wave 64 x 64: 200 registers, two workgroups per CU.  (MmaF32<2, 2, 2, 4>, 128 rows and half the
// question staging per row, was measured: 331 registers, one wave per SIMD, and no faster at 8 questions per album, 20 %
// slower at one -- DESIGN.md 4.1)
typedef MmaF32<1, 4, 2, 2> ShMma;
// the row types a kernel of this file may be instantiated with: fp32 anywhere, bf16 bits where they are used
template <class ROW, bool TRAIN, bool POOL>
constexpr bool sh_row_ok = std::is_same<ROW, float>::value || (std::is_same<ROW, bf16_t>::value && !TRAIN && POOL);
static_assert(ShMma::BM == SH_R && ShMma::BN == SH_BN && ShMma::NT == SH_NT && ShMma::TN % 2 == 0, "tile shape");

// ---- the plan.  One workgroup.  Indices are data: clamped before they address anything.
__device__ __forceinline__ int sh_album(const int* album, int i, int A) {
  const int a = album[i];
  return a < 0 ? 0 : (a >= A ? A - 1 : a);
}
// the album of reference i; POOL: -1 for an empty slot (any negative entry), which the plan passes over
template <bool POOL>
__device__ __forceinline__ int sh_ref_album(const int* album, int i, int A) {
  if constexpr (POOL) {
    const int a = album[i];
    return a < 0 ? -1 : (a >= A ? A - 1 : a);
  }
  return sh_album(album, i, A);
}
// The references (s.NR of them: the questions, POOL: the (question, slot) pairs) sorted by album and cut into groups.
// ORDERED (the training plan): the questions of an album stand in `order` by ascending question index, so that the
// backward's sum over an album's questions has ONE order, a function of `album` alone.  The cursor atomics below place a
// question wherever its atomic happens to arrive; here wave 0 alone walks the questions 64 at a time in ascending order,
// and per distinct album of a batch ONE lane advances that album's cursor by the number of the batch's questions about
// it, which take their places by lane rank.  Every cursor update is issued by a single wave in program order, one after
// the other: nothing depends on the order in which atomics of different waves arrive.  (An integer atomic is still the
// instruction, because it reads the cursor at L2, past this wave's own vector cache.)  ORDERED and POOL: the walk runs over
// the reference ids q M + m, so an album's references stand by ascending id; an empty slot joins no batch.
template <bool ORDERED, bool POOL = false>
__global__ __launch_bounds__(SH_PLAN_NT) void attn_shared_plan_kernel(ShShape s, ShWork wk, const int* __restrict__ album) {
  __shared__ int cell_c[SH_PLAN_NT], cell_g[SH_PLAN_NT];
  const int tid = threadIdx.x, A = s.A, NR = s.NR, G = s.G;
  for (int a = tid; a < A; a += SH_PLAN_NT) wk.acnt[a] = 0;
  __syncthreads();
  for (int i = tid; i < NR; i += SH_PLAN_NT) {
    const int a = sh_ref_album<POOL>(album, i, A);
    if (!POOL || a >= 0) atomicAdd(&wk.acnt[a], 1);
  }
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
    for (int base = 0; base < NR; base += 64) {
      const int i = base + tid;
      bool ok = i < NR;
      const int a = ok ? sh_ref_album<POOL>(album, i, A) : -1;
      if constexpr (POOL) {  // an empty slot: in no group, and out of the walk
        if (ok && a < 0) wk.qslot[i] = -1;
        ok = ok && a >= 0;
      }
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
    for (int i = tid; i < NR; i += SH_PLAN_NT) {
      const int a = sh_ref_album<POOL>(album, i, A);
      if (POOL && a < 0) {  // an empty slot: in no group
        wk.qslot[i] = -1;
        continue;
      }
      const int off = atomicAdd(&wk.acnt[a], 1);
      wk.order[wk.astart[a] + off] = i;
      wk.qslot[i] = (wk.agrp[a] + off / G) * G + off % G;
    }
  }
}

// ---- logits.  grid ngmax * K * ntile, 256 threads
// TRAIN: also the FIRST arg-max j of every row's maximum -> jmax [NQ,K,T] -- POOL: [NQ,K,M T], at the reference's slot --
// (compile-time: the inference kernel is unchanged).  TRAIN and TW: lin beside jmax, at the same address; r2 [A,K,T] at the
// album's own row, whichever reference's group computes it
// TW (compile-time too; tw_scale [NQ,T] -- POOL: [NQ,M T], read at the reference's slot -- else unused): the logits of the WARPED rows h' = s h, s = tw_scale[q,t], from the
// rows as they are held.  The scalar goes through the bilinear form: x = s (h.Qs + Rh.h) + s^2 (R2.h^2) + ct, cosine
// x = (h.Qn) s rsqrt(max(s^2 |h|^2, 1e-12)) -- the row pass keeps Rh.h and R2.h^2 (cosine: the raw sum h^2) apart, and
// the scales of the tile's rows for the group's questions are staged in LDS
// ROW (compile-time; float, or bf16_t: rows held as bf16 bits): how a row is LOADED, and nothing else -- ld4 / the staging
// widen four bf16 in registers, exactly, every lane keeps its channels, and from there on the kernel is the fp32 one on
// the widened rows: the same bits
template <int JT, bool TRAIN, bool TW, bool POOL = false, class ROW = float>
__global__ __launch_bounds__(SH_NT) void attn_shared_logits_kernel(ShShape s, ShWork wk, const ROW* __restrict__ hinfo,
                                                                  const uint8_t* __restrict__ hmask,
                                                                  const uint8_t* __restrict__ qmask,
                                                                  float* __restrict__ a_logits, ShTwArgs tw) {
  static_assert(sh_row_ok<ROW, TRAIN, POOL>, "bf16 rows: the pooled inference calls only");
  constexpr int JP = 32 * JT, G = SH_BN / JP;
  const float* __restrict__ tw_scale = tw.scale;
  __shared__ __attribute__((aligned(16))) float smem[ShMma::LDS_FLOATS];
  __shared__ float s_rt[SH_R], s_ct[SH_BN];
  // TW: s_rt holds Rh.h, s_r2 R2.h^2 (cosine: sum h^2); s_sc, s_s2 the factor of the product and the addend per (question, row)
  __shared__ float s_r2[TW ? SH_R : 1], s_sc[TW ? G : 1][TW ? SH_R : 1], s_s2[TW ? G : 1][TW ? SH_R : 1];
  __shared__ int s_q[G], s_o[POOL ? G : 1];  // a column block's question and -- POOL -- its slot's first position
  __shared__ uint8_t s_hv[SH_R], s_cv[SH_BN];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int tile = blockIdx.x % s.ntile, k = (blockIdx.x / s.ntile) % s.K, grp = blockIdx.x / (s.ntile * s.K);
  if (grp >= *wk.ngroups) return;
  const int4 gi = wk.grp[grp];
  const int a = gi.x, first = gi.y, cnt = gi.z;
  const int T = s.T, TP = sh_positions<POOL>(s), w = s.w, JQ = s.JQ, K = s.K, t0 = tile * SH_R;
  const size_t ak = (size_t)a * K + k;
  if (tid < G) {
    const int ref = tid < cnt ? wk.order[first + tid] : -1;
    s_q[tid] = ref < 0 ? -1 : sh_ref_q<POOL>(s, ref);
    if constexpr (POOL) s_o[tid] = ref < 0 ? 0 : sh_ref_off<POOL>(s, ref);
  }
  // (q, k, t) of column block g (whose question is q) in amax / jmax / lin, and times JQ in a_logits
  auto at_of = [&](int q, int g, int t) -> size_t { return ((size_t)q * K + k) * TP + (POOL ? s_o[g] : 0) + t; };
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
      const size_t at = at_of(s_q[e / rows], e / rows, t0 + e % rows);
      wk.amax[at] = FVTA_NEG;
      if constexpr (TRAIN) wk.jmax[at] = 0;
      if constexpr (TRAIN && TW) tw.lin[at] = 0.f;  // (no gradient passes through a masked logit: written, never used)
    }
    if constexpr (TRAIN && TW)
      if (grp == wk.agrp[a])
        for (int e = tid; e < rows; e += SH_NT) tw.r2[ak * T + t0 + e] = 0.f;
    if (a_logits)
      for (int g = 0; g < cnt; ++g) {
        float* dst = a_logits + at_of(s_q[g], g, t0) * JQ;
        for (int e = tid; e < rows * JQ; e += SH_NT) dst[e] = FVTA_NEG;
      }
    return;
  }
  const ROW* hbase = hinfo + ak * T * w;
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
        s_sc[e / SH_R][e % SH_R] = (q >= 0 && t < T) ? tw_scale[(size_t)q * TP + (POOL ? s_o[e / SH_R] : 0) + t] : 0.f;
      }
  }
  ShMma mma;
  mma.init(tid);
  StageKContig<SH_R, ShMma::BK, SH_NT, ShMma::LDA> sa;
  StageKContig<SH_BN, ShMma::BK, SH_NT, ShMma::LDB> sb;
  auto fa = [&](int r, int kk, bool& ok) -> const ROW* {
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
        if (a_logits && live && t < T) a_logits[at_of(q, col / JP, t) * JQ + j] = v;
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
        if (mma.l31 == r && q >= 0 && t < T) wk.amax[at_of(q, mma.col_of(jn) / JP, t)] = m;
        if constexpr (TRAIN) {  // columns of a lane: j = l31 (and 32 + l31); a dead column holds -inf and never equals m
          int jm = mx[jn][r] == m ? mma.l31 : 255;
          if (JT == 2 && jm == 255 && mx[jn + 1][r] == m) jm = 32 + mma.l31;
#pragma unroll
          for (int o = 16; o > 0; o >>= 1) jm = min(jm, __shfl_xor(jm, o, 64));
          if (mma.l31 == r && q >= 0 && t < T) wk.jmax[at_of(q, mma.col_of(jn) / JP, t)] = (uint8_t)min(jm, JQ - 1);
          if constexpr (TW) {  // lin at the winner: the one lane that holds column jm puts it in, 31 zeros are added to it
            const int mine = mx[jn][r] == m ? mma.l31 : ((JT == 2 && mx[jn + 1][r] == m) ? 32 + mma.l31 : 255);
            const float acc = (JT == 2 && mine >= 32) ? mma.acc[i][JT == 2 ? jn + 1 : jn][r] : mma.acc[i][jn][r];
            float lv = (mine == jm && jm != 255) ? acc + s_rt[mma.row_of(i, r)] : 0.f;
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) lv += __shfl_xor(lv, o, 64);
            if (mma.l31 == r && q >= 0 && t < T) tw.lin[at_of(q, mma.col_of(jn) / JP, t)] = lv;
          }
        }
      }
    }
  }
}

// ---- weighted sums.  grid ngmax * K * S, 256 threads: thread tid owns channels 4 tid .. + 3 (+ 1024 per further CPT)
// TW (compile-time; tw_scale [NQ,T] -- POOL: [NQ,M T] -- else unused): the sum runs over the warped rows s h: the staged weight carries s
// ROW: as the logits kernel's -- with bf16 rows the further CPT's offset of 1024 counts 2-byte elements
template <int G, int CPT, bool TW, bool POOL = false, class ROW = float>
__global__ __launch_bounds__(256) void attn_shared_wsum_kernel(ShShape s, ShWork wk, const ROW* __restrict__ hinfo,
                                                               const float* __restrict__ tw_scale) {
  static_assert(sh_row_ok<ROW, false, POOL>, "bf16 rows: the pooled calls only");
  __shared__ float s_p[SH_CH][G], s_M[G], s_cf[G];
  __shared__ int s_q[G], s_o[POOL ? G : 1];  // as the logits kernel's
  const int tid = threadIdx.x;
  const int sp = blockIdx.x % s.S, k = (blockIdx.x / s.S) % s.K, grp = blockIdx.x / (s.S * s.K);
  if (grp >= *wk.ngroups) return;
  const int4 gi = wk.grp[grp];
  const int a = gi.x, first = gi.y, cnt = gi.z;
  const int T = s.T, TP = sh_positions<POOL>(s), w = s.w, K = s.K;
  if (tid < G) {
    const int ref = tid < cnt ? wk.order[first + tid] : -1;
    const int q = ref < 0 ? -1 : sh_ref_q<POOL>(s, ref);
    s_q[tid] = q;
    if constexpr (POOL) s_o[tid] = ref < 0 ? 0 : sh_ref_off<POOL>(s, ref);
    s_M[tid] = q >= 0 ? wk.M[(size_t)q * K + k] : 0.f;
    s_cf[tid] = q >= 0 ? wk.coef[(size_t)q * K + k] : 0.f;
  }
  f32x4 acc[G][CPT];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int i = 0; i < CPT; ++i) acc[g][i] = zero4();
  const int tb = sp * s.rps, te = min(T, tb + s.rps);
  const ROW* hbase = hinfo + ((size_t)a * K + k) * T * w;
  const bool mine = 4 * tid < w;
  for (int c0 = tb; c0 < te; c0 += SH_CH) {
    __syncthreads();
    for (int e = tid; e < SH_CH * G; e += 256) {
      const int g = e / SH_CH, r = e % SH_CH, t = c0 + r, q = s_q[g];
      float p = (t < te && q >= 0) ? expf(wk.amax[((size_t)q * K + k) * TP + (POOL ? s_o[g] : 0) + t] - s_M[g]) : 0.f;
      if constexpr (TW) p = (t < te && q >= 0) ? p * tw_scale[(size_t)q * TP + (POOL ? s_o[g] : 0) + t] : 0.f;
      s_p[r][g] = p;
    }
    __syncthreads();
    const int nr = min(SH_CH, te - c0);
    if (mine) {
#pragma unroll 4
      for (int r = 0; r < nr; ++r) {
        const ROW* row = hbase + (size_t)(c0 + r) * w + 4 * tid;
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

template <int G, bool TW, bool POOL = false, class ROW = float>
static void sh_launch_wsum(const ShShape& s, const ShWork& wk, const ROW* hinfo, const float* tw_scale, hipStream_t st) {
  const dim3 grid((unsigned)((int64_t)s.ngmax * s.K * s.S));
  if (s.w <= 1024)
    hipLaunchKernelGGL((attn_shared_wsum_kernel<G, 1, TW, POOL, ROW>), grid, dim3(256), 0, st, s, wk, hinfo, tw_scale);
  else
    hipLaunchKernelGGL((attn_shared_wsum_kernel<G, 2, TW, POOL, ROW>), grid, dim3(256), 0, st, s, wk, hinfo, tw_scale);
}

}  // namespace fvta
