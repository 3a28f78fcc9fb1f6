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
// copy attn_bwd.hip runs too; the row and question passes (2, 3) are this file's own.
#include "attn_shared_common.h"
#include "attn_bwd_shared.h"

namespace fvta {

constexpr int SHB_CS = 32;            // channels per slice of the question pass
constexpr int SHB_JG = ATTN_BWD_JG;   // question positions per workgroup of the fold
constexpr int SHB_ROW_WGS = 1024;     // about this many workgroups of the row pass (then several tiles per workgroup)
constexpr int SHB_Q_WAVES = 1280;     // about this many waves of the question pass (5 x 32 KB of LDS per CU)

struct ShBwdShape {
  int TPR, CPT, RH, RPT, TR;  // row pass: threads per row, float4 per thread and row, row groups, rows per thread, tile rows
  int ntb, tpw, nch;          // row tiles per (album, k), tiles per workgroup, workgroups per (album, k)
  int nsl, TS, rps;           // question pass: channel slices, T splits, rows per split
  int JZ;                     // fold: groups of SHB_JG question positions
};

static ShBwdShape shb_shape(const ShShape& s) {
  ShBwdShape b;
  b.TPR = s.w / 4 < 256 ? s.w / 4 : 256;
  b.CPT = s.w / (4 * b.TPR);
  b.RH = 256 / b.TPR;
  b.RPT = b.CPT == 1 ? 8 : 4;
  b.TR = b.RH * b.RPT;
  b.ntb = (s.T + b.TR - 1) / b.TR;
  const int64_t tiles = (int64_t)s.A * s.K * b.ntb;
  int64_t tpw = (tiles + SHB_ROW_WGS - 1) / SHB_ROW_WGS;
  if (tpw > b.ntb) tpw = b.ntb;
  if (tpw < 1) tpw = 1;
  b.tpw = (int)tpw;
  b.nch = (b.ntb + b.tpw - 1) / b.tpw;
  b.nsl = s.w / SHB_CS;
  int64_t ts = (SHB_Q_WAVES + (int64_t)s.ngmax * b.nsl - 1) / ((int64_t)s.ngmax * b.nsl);
  const int maxs = (s.T + 63) / 64;
  if (ts > maxs) ts = maxs;
  if (ts < 1) ts = 1;
  b.rps = (int)((s.T + ts - 1) / ts);
  b.TS = (s.T + b.rps - 1) / b.rps;
  b.JZ = (s.JQ + SHB_JG - 1) / SHB_JG;
  return b;
}

struct ShBwdWork {
  float *coef, *gu, *dss;  // [NQ,K]: r / L, g.u[k], ds[k] / ties (0 for a fully masked (question, k))
  float* dx;               // [NQ,K,T] gradient of the row's winning logit
  float* qpart;            // [ngmax][TS][G JP = 256][w]  dQs partials
  float* dctp;             // [ngmax][TS][256]            d ct partials
  float* rowp;             // [A K nch][RH][2][w]         d Rh, d R2 partials
  float* pvec;             // [NQ JZ][3][w]               d U, d Cq, d C2 partials
  float* dctn;             // [NQ][JP]
  size_t bytes;
  ShBwdWork(const ShShape& s, const ShBwdShape& b, void* p) {
    FvtaCarver c(p);
    const size_t nk = (size_t)s.NQ * s.K;
    coef = c.take<float>(nk);
    gu = c.take<float>(nk);
    dss = c.take<float>(nk);
    dx = c.take<float>(nk * s.T);
    qpart = c.take<float>((size_t)s.ngmax * b.TS * SH_BN * s.w);
    dctp = c.take<float>((size_t)s.ngmax * b.TS * SH_BN);
    rowp = c.take<float>((size_t)s.A * s.K * b.nch * b.RH * 2 * s.w);
    pvec = c.take<float>((size_t)s.NQ * b.JZ * 3 * s.w);
    dctn = c.take<float>((size_t)s.NQ * s.JP);
    bytes = c.off;
  }
};

// ---- per-(question, k) scalars: attn_bwd_shared.h's prep body on the shared forward's `saved`.  grid NQ; a wave per k
__global__ __launch_bounds__(1024) void attn_shared_bwd_prep_kernel(ShShape s, ShWork sv, ShBwdWork wk,
                                                                   const float* __restrict__ d_h_a) {
  const size_t q = blockIdx.x, qk = q * s.K;
  // a (question, k) without a valid (t, j) pair has M = -1e30: nothing passes into its masked logits
  const bool allmasked = (int)threadIdx.x < s.K && sv.M[qk + threadIdx.x] == FVTA_NEG;
  attn_bwd_prep_body(d_h_a + q * s.w, sv.u + qk * s.w, sv.M + qk, sv.amax + qk * s.T, sv.r + qk, sv.L + qk, allmasked, s.w, s.K,
                     s.T, wk.coef + qk, wk.gu + qk, wk.dss + qk);
}

// ---- row pass.  grid A K nch, 256 threads = RH row groups x TPR threads; a thread holds RPT rows x CPT float4
template <int TPR, int CPT, int RPT>
__global__ __launch_bounds__(256) void attn_shared_bwd_rows_kernel(ShShape s, ShBwdShape bs, ShWork sv, ShBwdWork wk,
                                                                  const float* __restrict__ hinfo,
                                                                  const float* __restrict__ d_h_a,
                                                                  float* __restrict__ d_hinfo) {
  constexpr int RH = 256 / TPR, TR = RH * RPT;
  constexpr int WPR = TPR >= 64 ? TPR / 64 : 1;  // waves that share a row
  __shared__ float s_dot[4][TR], s_pr[TR], s_dx[TR];
  __shared__ int s_jj[TR];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int cq = tid % TPR, rh = tid / TPR;
  const int ch = blockIdx.x % bs.nch, ak = blockIdx.x / bs.nch, a = ak / s.K, k = ak % s.K;
  const int T = s.T, w = s.w, K = s.K, JP = s.JP;
  const int q0 = min(max(sv.astart[a], 0), s.NQ), nqa = min(sv.acnt[a], s.NQ - q0);  // (the plan's own numbers; bounded all the same)
  const float* __restrict__ hbase = hinfo + (size_t)ak * T * w;
  float* __restrict__ dhbase = d_hinfo + (size_t)ak * T * w;
  f32x4 rh4[CPT], r24[CPT], accRh[CPT], accR2[CPT];
#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    rh4[c] = ld4(sv.vecs + VEC_RH * w + 4 * (cq + c * TPR));
    r24[c] = ld4(sv.vecs + VEC_R2 * w + 4 * (cq + c * TPR));
    accRh[c] = accR2[c] = zero4();
  }
  const int tile_end = min(bs.ntb, (ch + 1) * bs.tpw);
  for (int tile = ch * bs.tpw; tile < tile_end; ++tile) {
    const int t0 = tile * TR;
    f32x4 h[RPT][CPT], dh[RPT][CPT];
    float sdx[RPT];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int t = t0 + rh * RPT + i;
      sdx[i] = 0.f;
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        h[i][c] = t < T ? ld4(hbase + (size_t)t * w + 4 * (cq + c * TPR)) : zero4();
        dh[i][c] = zero4();
      }
    }
    for (int qi = 0; qi < nqa; ++qi) {
      int q = sv.order[q0 + qi];
      q = q < 0 ? 0 : (q >= s.NQ ? s.NQ - 1 : q);
      f32x4 gv[CPT];
#pragma unroll
      for (int c = 0; c < CPT; ++c) gv[c] = ld4(d_h_a + (size_t)q * w + 4 * (cq + c * TPR));
      // g.h[t]: over the TPR threads of a row
#pragma unroll
      for (int i = 0; i < RPT; ++i) {
        float v = 0.f;
#pragma unroll
        for (int c = 0; c < CPT; ++c) {
          const f32x4 pd = h[i][c] * gv[c];
          v += (pd[0] + pd[1]) + (pd[2] + pd[3]);
        }
#pragma unroll
        for (int o = 1; o < (TPR < 64 ? TPR : 64); o <<= 1) v += __shfl_xor(v, o, 64);
        if (TPR >= 64) {
          if (lane == 0) s_dot[wave][rh * RPT + i] = v;
        } else {
          if (cq == 0) s_dot[0][rh * RPT + i] = v;
        }
      }
      __syncthreads();
      if (tid < TR) {
        const int t = t0 + tid;
        float pr = 0.f, dx = 0.f;
        int j = 0;
        if (t < T) {
          float gh = 0.f;
          if (TPR >= 64) {
            const int rgp = tid / RPT;  // row `tid` belongs to row group rgp, whose waves are [rgp WPR, rgp WPR + WPR)
#pragma unroll
            for (int v = 0; v < WPR; ++v) gh += s_dot[rgp * WPR + v][tid];
          } else {
            gh = s_dot[0][tid];
          }
          const size_t qk = (size_t)q * K + k;
          const float M = sv.M[qk], am = sv.amax[qk * T + t];
          pr = expf(am - M) * wk.coef[qk];
          // pr = 0: a masked row beside valid ones (its g.h may be anything), or r underflowed (then ds is 0 as well)
          if (pr != 0.f && M != FVTA_NEG) {
            const float damax = pr * (gh - wk.gu[qk]) + (am == M ? wk.dss[qk] : 0.f);
            dx = s.add_tanh ? damax * (1.f - am * am) : damax;
          }
          j = min((int)sv.jmax[qk * T + t], JP - 1);
          wk.dx[qk * T + t] = dx;
        }
        s_pr[tid] = pr;
        s_dx[tid] = dx;
        s_jj[tid] = j;
      }
      __syncthreads();
      const float* __restrict__ Qs = sv.Qs + (size_t)q * JP * w;
#pragma unroll
      for (int i = 0; i < RPT; ++i) {
        const int row = rh * RPT + i;
        const float pr = s_pr[row], dx = s_dx[row];
#pragma unroll
        for (int c = 0; c < CPT; ++c) dh[i][c] += gv[c] * pr;
        if (dx != 0.f) {
          const int j = s_jj[row];
#pragma unroll
          for (int c = 0; c < CPT; ++c) {
            const f32x4 qs = ld4(Qs + (size_t)j * w + 4 * (cq + c * TPR));
            dh[i][c] += (qs + rh4[c] + r24[c] * h[i][c] * 2.f) * dx;
          }
          sdx[i] += dx;
        }
      }
      // (the next question's s_dot is written after this barrier pair, its s_pr / s_dx after the next first barrier, which
      // every thread reaches only when it is through with the reads above)
    }
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int t = t0 + rh * RPT + i;
      if (t < T) {
#pragma unroll
        for (int c = 0; c < CPT; ++c) {
          *reinterpret_cast<f32x4*>(dhbase + (size_t)t * w + 4 * (cq + c * TPR)) = dh[i][c];
          if (sdx[i] != 0.f) {
            accRh[c] += h[i][c] * sdx[i];
            accR2[c] += h[i][c] * h[i][c] * sdx[i];
          }
        }
      }
    }
    __syncthreads();  // the tile's last reads of s_pr / s_dx / s_jj before the next tile's first question
  }
  float* __restrict__ rowp = wk.rowp + ((size_t)blockIdx.x * RH + rh) * 2 * w;
#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    *reinterpret_cast<f32x4*>(rowp + 4 * (cq + c * TPR)) = accRh[c];
    *reinterpret_cast<f32x4*>(rowp + w + 4 * (cq + c * TPR)) = accR2[c];
  }
}

// ---- question pass.  grid ngmax TS nsl, 64 threads: lane = (question g of the group, 4 of the slice's 32 channels)
template <int G>
__global__ __launch_bounds__(64) void attn_shared_bwd_q_kernel(ShShape s, ShBwdShape bs, ShWork sv, ShBwdWork wk,
                                                              const float* __restrict__ hinfo) {
  constexpr int JP = SH_BN / G, C4 = SHB_CS / 4;
  __shared__ f32x4 s_acc[SH_BN][C4];
  __shared__ float s_dct[SH_BN];
  const int tid = threadIdx.x;
  const int sl = blockIdx.x % bs.nsl, ts = (blockIdx.x / bs.nsl) % bs.TS, grp = blockIdx.x / (bs.nsl * bs.TS);
  if (grp >= *sv.ngroups) return;
  const int4 gi = sv.grp[grp];
  const int a = min(max(gi.x, 0), s.A - 1), first = gi.y, cnt = min(max(gi.z, 0), G);
  const int T = s.T, w = s.w, K = s.K;
  for (int e = tid; e < SH_BN * C4; e += 64) (&s_acc[0][0])[e] = zero4();
  for (int e = tid; e < SH_BN; e += 64) s_dct[e] = 0.f;
  __syncthreads();
  // A group with fewer than G questions leaves accumulator regions free: `rep` lane groups then share a question, each
  // taking every rep-th run of four rows into a region of its own, and the regions are added in region order on the way
  // out.  rep depends on the group's count alone.
  const int rep = cnt > 0 ? max(G / cnt, 1) : 1;
  const int gl = tid / C4, c4 = tid % C4;                  // lane group = accumulator region
  const int g = cnt > 0 ? gl % cnt : 0, part = cnt > 0 ? gl / cnt : 0;
  int q = (gl < G && cnt > 0 && part < rep && g < cnt && first + g < s.NQ) ? sv.order[first + g] : -1;
  if (q >= s.NQ) q = -1;
  const int tb = ts * bs.rps, te = min(T, tb + bs.rps);
  if (q >= 0 && tb < te) {
    for (int k = 0; k < K; ++k) {
      const float* __restrict__ hrow = hinfo + ((size_t)a * K + k) * T * w + sl * SHB_CS + 4 * c4;
      const float* __restrict__ dxp = wk.dx + ((size_t)q * K + k) * T;
      const uint8_t* __restrict__ jp = sv.jmax + ((size_t)q * K + k) * T;
      for (int t4 = tb + 4 * part; t4 < te; t4 += 4 * rep) {  // four rows in flight
        float dx[4];
        int j[4];
        f32x4 h[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int t = min(t4 + i, te - 1);
          dx[i] = t4 + i < te ? dxp[t] : 0.f;
          j[i] = min((int)jp[t], JP - 1);
          h[i] = ld4(hrow + (size_t)t * w);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (dx[i] != 0.f) {
            s_acc[gl * JP + j[i]][c4] += h[i] * dx[i];
            if (sl == 0 && c4 == 0) s_dct[gl * JP + j[i]] += dx[i];
          }
      }
    }
  }
  __syncthreads();
  const size_t slot = (size_t)grp * bs.TS + ts;
  float* __restrict__ dst = wk.qpart + slot * SH_BN * w + sl * SHB_CS;
  for (int e = tid; e < SH_BN * C4; e += 64) {
    const int row = e / C4, cc = e % C4, gs = row / JP, j = row % JP;
    f32x4 v = zero4();
    if (gs < cnt)
      for (int p = 0; p < rep; ++p) v += s_acc[(gs + cnt * p) * JP + j][cc];
    *reinterpret_cast<f32x4*>(dst + (size_t)row * w + 4 * cc) = v;
  }
  if (sl == 0)
    for (int e = tid; e < SH_BN; e += 64) {
      const int gs = e / JP, j = e % JP;
      float v = 0.f;
      if (gs < cnt)
        for (int p = 0; p < rep; ++p) v += s_dct[(gs + cnt * p) * JP + j];
      wk.dctp[slot * SH_BN + e] = v;
    }
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

// 0: fine, else the status with the message set
static int shb_check(const fvta_attn_shared_desc* d, const char* who) {
  if (int e = fvta_attn_shared_check_train(d, who)) return e;
  const ShShape s = sh_shape(d);
  const ShBwdShape b = shb_shape(s);
  if ((int64_t)s.A * s.K * b.nch > 0x7fffffff || (int64_t)s.ngmax * b.TS * b.nsl > 0x7fffffff) {
    fvta_set_error("%s: unsupported shape (A=%d NQ=%d K=%d T=%d JQ=%d w=%d): too many workgroups", who, d->A, d->NQ, d->K, d->T,
                   d->JQ, d->w);
    return FVTA_ERR_UNSUPPORTED;
  }
  return FVTA_OK;
}

}  // namespace fvta
using namespace fvta;

extern "C" size_t fvta_attn_shared_bwd_workspace_bytes(const fvta_attn_shared_desc* d) {
  if (shb_check(d, "attn_shared_bwd_workspace_bytes") != FVTA_OK) return 0;
  const ShShape s = sh_shape(d);
  return ShBwdWork(s, shb_shape(s), nullptr).bytes;
}

extern "C" int fvta_attn_shared_bwd_plan(const fvta_attn_shared_desc* d, int32_t out[4]) {
  if (int e = shb_check(d, "attn_shared_bwd_plan")) return e;
  FVTA_CHECK_ARG(out != nullptr, "attn_shared_bwd_plan: null pointer");
  const ShBwdShape b = shb_shape(sh_shape(d));
  out[0] = b.TR;
  out[1] = b.TS;
  out[2] = SHB_CS;
  out[3] = b.tpw;
  return FVTA_OK;
}

extern "C" int fvta_attn_shared_bwd(const fvta_attn_shared_desc* d, const float* hinfo, const uint8_t* hmask, const float* hq,
                                    const uint8_t* qmask, const int32_t* album, const float* W, const float* b,
                                    const float* d_h_a, const void* saved, float* d_hinfo, float* d_hq, float* dW, float* db,
                                    void* workspace, fvta_stream_t stream_) {
  if (int e = shb_check(d, "attn_shared_bwd")) return e;
  FVTA_CHECK_ARG(hinfo && hq && album && d_h_a && saved && d_hinfo && d_hq && dW && db && workspace,
                 "attn_shared_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream_;
  ShShape s = sh_shape(d);
  s.use_mask = (hmask && qmask) ? 1 : 0;
  const ShBwdShape bs = shb_shape(s);
  const ShWork sv(s, const_cast<void*>(saved), nullptr);
  const ShBwdWork wk(s, bs, workspace);
  hipLaunchKernelGGL(attn_shared_bwd_prep_kernel, dim3(s.NQ), dim3(s.K > 4 ? 1024 : 256), 0, st, s, sv, wk, d_h_a);
  const dim3 rgrid((unsigned)((int64_t)s.A * s.K * bs.nch));
#define FVTA_SHB_ROWS(TPR, CPT, RPT) \
  hipLaunchKernelGGL((attn_shared_bwd_rows_kernel<TPR, CPT, RPT>), rgrid, dim3(256), 0, st, s, bs, sv, wk, hinfo, d_h_a, d_hinfo)
  switch (s.w) {
    case 64: FVTA_SHB_ROWS(16, 1, 8); break;
    case 128: FVTA_SHB_ROWS(32, 1, 8); break;
    case 256: FVTA_SHB_ROWS(64, 1, 8); break;
    case 512: FVTA_SHB_ROWS(128, 1, 8); break;
    case 1024: FVTA_SHB_ROWS(256, 1, 8); break;
    default: FVTA_SHB_ROWS(256, 2, 4); break;
  }
#undef FVTA_SHB_ROWS
  const dim3 qgrid((unsigned)((int64_t)s.ngmax * bs.TS * bs.nsl));
  if (s.G == 8)
    hipLaunchKernelGGL(attn_shared_bwd_q_kernel<8>, qgrid, dim3(64), 0, st, s, bs, sv, wk, hinfo);
  else
    hipLaunchKernelGGL(attn_shared_bwd_q_kernel<4>, qgrid, dim3(64), 0, st, s, bs, sv, wk, hinfo);
  hipLaunchKernelGGL(attn_shared_bwd_fold_kernel, dim3(s.NQ, (s.w + 255) / 256, bs.JZ), dim3(256), 0, st, s, bs, sv, wk, hq, d_hq);
  hipLaunchKernelGGL(attn_shared_bwd_params_kernel, dim3((s.w + 63) / 64 + 1), dim3(256), 0, st, s, bs, wk, dW, db);
  FVTA_CHECK_LAUNCH("attn_shared_bwd");
  return FVTA_OK;
}
